"""The MXFP8 forward route (BERT_HIP_MX=fp8 at load, the key "mx"): which kernels a pass runs, that a sentence's bits do not depend on its
batch, the host and device entry points, capture and replay, and how far the embeddings move from the f16 route's in the same context.
Worst cosine between the two routes over the sentences below, measured on an MI355X: 0.996828 (MEASURED_COS); the floor is 1 - 2 (1 - that)."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from conftest import cosine
from test_gpu_stream_capture import _captured, _cu, _eager, _replay, _same, hip  # noqa: F401 (hip: the fixture)

pytestmark = pytest.mark.gpu
MEASURED_COS = 0.996828
FLOOR = 1 - 2 * (1 - MEASURED_COS)
LENS = [1, 64, 33, 17, 64, 5, 40, 64]                          # 1 and the position limit among them; 288 tokens: two token tiles
FUSED = ("qkv_attention2", "layer_tail", "model_kernel")


def load(make_model, mx):
    path, hp = make_model("tiny-h128", "f16", 1)
    with pytest.MonkeyPatch.context() as mp:
        if mx:
            mp.setenv("BERT_HIP_MX", "fp8")
        else:
            mp.delenv("BERT_HIP_MX", raising=False)
        return pybert.BertModel(path), hp


@pytest.fixture(scope="module")
def mx_model(make_model):
    m, hp = load(make_model, True)
    sents = [gf.synthetic_token_ids(1, n, hp.n_vocab, seed=70 + i)[0] for i, n in enumerate(LENS)]
    yield m, hp, sents
    m.close()


def kernels_of(m, sents):
    m.profile(True)
    out = m.eval_packed(np.concatenate(sents), _cu(LENS))
    rep = m.profile_report(families=True)
    m.profile(False)
    return out, rep


def test_the_switch_selects_the_kernels(mx_model):
    m, hp, sents = mx_model
    on, rep = kernels_of(m, sents)
    assert "family:gemm_mx" in rep and rep["mx_quantize"]["launches"] == 3 * hp.n_layer and not any(k in rep for k in FUSED)
    assert rep["family:gemm_mx"]["launches"] == 4 * hp.n_layer
    m.set_option("mx", "0")
    off, rep = kernels_of(m, sents)
    m.set_option("mx", "1")
    assert "family:gemm_mx" not in rep and "mx_quantize" not in rep and any(k in rep for k in FUSED)
    # quality: the f16 route of the same context is the reference
    cos = [cosine(a, b) for a, b in zip(on, off)]
    print(f"measured: worst cosine mx = 1 against mx = 0: {min(cos):.6f}")
    assert np.isfinite(on).all() and min(cos) >= FLOOR


def test_a_sentence_alone_has_its_bits_of_the_batch(mx_model):
    m, hp, sents = mx_model
    batch = m.eval_packed(np.concatenate(sents), _cu(LENS))
    for i in (0, 1, 2, 7):
        assert _same(m.eval_packed(sents[i], _cu(LENS[i:i + 1]))[0], batch[i]), i


def test_device_entry_capture_and_replays(mx_model, hip):
    m, hp, sents = mx_model
    toks, cu = np.concatenate(sents).astype(np.int32), _cu(LENS)
    B, T, H = len(LENS), int(cu[-1]), hp.n_embd
    host = m.eval_packed(toks, cu)
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.nans((B, H))
    out, s = [(d_out, (B, H), np.float32)], hip.stream()
    m.reserve(T, B)
    call = lambda: m.lib.bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max(LENS), d_out, s)
    (E,) = _eager(hip, call, out)
    assert m.check() == 0 and _same(E, host)
    graph, ex = _captured(hip, s, call, out)
    for i in range(2):
        (got,) = _replay(hip, ex, s, out)
        assert _same(got, E), i
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_out)


def test_without_the_images_the_key_is_refused(make_model, mx_model, capfd):
    m, hp = load(make_model, False)
    sents = mx_model[2]
    base, rep = kernels_of(m, sents)
    capfd.readouterr()
    m.set_option("mx", "1")
    assert "ignored" in capfd.readouterr().err
    again, rep2 = kernels_of(m, sents)
    assert _same(again, base) and "family:gemm_mx" not in rep and "family:gemm_mx" not in rep2
    m.close()
