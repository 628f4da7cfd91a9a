"""CPU-side tests of the relative position bias (MPNet models): the bucket function and the expanded table against HuggingFace's, the
float64 model of rel_bias_reference.py against transformers' MPNetModel, the model file's new tensor, the tokenizer's <s> / </s>, and
the new entry points without a device."""
import dataclasses
import os

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import rel_bias_reference as rb

TINY = gf.BertHParams(64, 64, 64, 128, 2, 2)


def _write(path, hp=TINY, ftype="f16", rel_bias=True, vocab=None, weights=None, seed=3):
    w = weights if weights is not None else gf.synthetic_weights(hp, seed, rel_bias=rel_bias)
    gf.write_model(str(path), hp, w, gf.FTYPE_BY_NAME[ftype], vocab=vocab)
    return str(path)


# ------------------------------------------------------------------------------------------------
# bucket and table
# ------------------------------------------------------------------------------------------------
def test_bucket_edges():
    d = np.array([0, -1, 1, -7, 7, -8, 8, -11, 12, 15, 16, 22, 23, 31, 32, 45, 46, 63, 64, 90, 91, 511, -511])
    want = [0, 1, 17, 7, 23, 8, 24, 8, 25, 25, 26, 26, 27, 27, 28, 28, 29, 29, 30, 30, 31, 31, 15]
    assert rb.bucket(d).tolist() == want
    assert 16 not in rb.bucket(np.arange(-600, 601))


def test_bucket_matches_transformers():
    torch = pytest.importorskip("torch")
    mpnet = pytest.importorskip("transformers.models.mpnet.modeling_mpnet")
    P = rb.P_LONG                                    # (+-1151: the longest table the matrix-core launcher can serve)
    d = np.arange(-(P - 1), P)
    got = mpnet.MPNetEncoder.relative_position_bucket(torch.tensor(d), num_buckets=32, max_distance=128).numpy()
    assert np.array_equal(got, rb.bucket(d))


@pytest.mark.parametrize("n_head,P", [(1, 1), (2, 7), (12, 512), (3, 514), (2, 128), (2, 1152)])
def test_host_expansion_is_the_table(n_head, P):
    W = rb.draw_W(n_head, seed=n_head)
    got = pybert.test_rel_bias_table(W, P)
    assert got.shape == (n_head, 2 * P - 1) and np.array_equal(got, rb.rel_table(W, P))
    assert np.array_equal(got[:, P - 1], W[0])                # distance 0


def test_float64_model_matches_transformers(tmp_path):
    """rel_bias_reference.Model on a file written through hf_mpnet_weights against transformers' MPNetModel in double, position rows
    from 2 on.  (gelu_new: the engine's GELU is ggml's tanh form.)"""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    hp = gf.BertHParams(100, 40, 64, 128, 2, 2)
    cfg = tr.MPNetConfig(vocab_size=hp.n_vocab, hidden_size=64, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                         max_position_embeddings=hp.n_max_tokens + 2, hidden_act="gelu_new", layer_norm_eps=1e-5,
                         hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = tr.MPNetModel(cfg, add_pooling_layer=False).double().eval()
    # our synthetic weights, through the inverse mapping, so that the table and the biases are not at their initial values
    ours = gf.synthetic_weights(hp, 11, rel_bias=True)
    sd = {k: torch.tensor(v, dtype=torch.float64) for k, v in rb.mpnet_state_dict(ours).items()}
    missing = hf.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    back = gf.hf_mpnet_weights(hf.state_dict(), hp.n_layer)
    assert set(back) == set(ours) and all(np.array_equal(back[k], ours[k]) for k in ours if "token_type" not in k)
    assert not back["embeddings.token_type_embeddings.weight"].any()
    path = _write(tmp_path / "m.bin", hp, "f32", weights=back)
    ref = rb.Model(path)
    rng = np.random.default_rng(0)
    for n in (1, 9, 13, 40):
        ids = rng.integers(3, hp.n_vocab, size=n)                 # (not 1: MPNet's padding id takes no position)
        with torch.no_grad():
            want = hf(input_ids=torch.tensor(ids)[None]).last_hidden_state[0].numpy()
        got = ref.hidden(ids)[-1]
        assert np.abs(got - want).max() < 1e-9 * max(1.0, np.abs(want).max()), n


# ------------------------------------------------------------------------------------------------
# the model file
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ftype", ["f32", "f16", "q4_0"])
def test_a_file_with_the_tensor_loads(tmp_path, ftype):
    vocab = gf.synthetic_vocab(TINY.n_vocab)
    vocab[0], vocab[2] = b"<s>", b"</s>"
    with_t = _write(tmp_path / "with.bin", ftype=ftype, vocab=vocab)
    without = _write(tmp_path / "without.bin", ftype=ftype, rel_bias=False, vocab=vocab)
    mf = gf.read_model(with_t)
    t, shp, _ = mf.raw[gf.REL_BIAS_NAME]
    assert shp == (32, TINY.n_head) and t == (gf.FTYPE_F16 if ftype == "f16" else gf.FTYPE_F32)      # never quantised
    a = pybert.BertModel(with_t, tokenizer_only=True)
    b = pybert.BertModel(without, tokenizer_only=True)
    assert a.relative_attention is True and b.relative_attention is False
    assert pybert.lib().bert_hip_relative_attention(a.ctx) == 1 and pybert.lib().bert_hip_relative_attention(b.ctx) == 0
    a.close(); b.close()


def test_the_full_parse_takes_the_tensor(tmp_path, capfd):
    """ModelFile::load on the whole file (pybert.model_digest needs no device): the tensor is accepted alone and behind either head;
    31 buckets and a wrong head count are refused with a message.  On the parent commit the tensor is an unknown one."""
    hp = TINY
    for kw in ({}, {"n_labels": 2}, {"mlm_head": True}, {"n_labels": 1, "mlm_head": True}):
        w = gf.synthetic_weights(hp, 3, rel_bias=True, **kw)
        n, legacy, _ = pybert.model_digest(_write(tmp_path / "m.bin", weights=w))
        assert n == len(w) and not legacy, kw
    w = gf.synthetic_weights(hp, 3, rel_bias=True)
    w[gf.REL_BIAS_NAME] = w[gf.REL_BIAS_NAME][:31]
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        pybert.model_digest(_write(tmp_path / "b31.bin", weights=w))
    err = capfd.readouterr().err
    assert "31 relative position buckets" in err and "32" in err, err
    w[gf.REL_BIAS_NAME] = np.zeros((32, hp.n_head + 1), dtype=np.float32)
    with pytest.raises(RuntimeError):
        pybert.model_digest(_write(tmp_path / "heads.bin", weights=w))
    assert "wrong shape" in capfd.readouterr().err


def test_quantize_tool_copies_the_tensor(tmp_path):
    """bert-quantize leaves the table as it is (f16 here) and the quantised file loads"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "bert.cpp_amd", "bin", "bert-quantize")
    src = _write(tmp_path / "f16.bin")
    dst = str(tmp_path / "q4_0.bin")
    r = subprocess.run([exe, src, dst, "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    a, b = gf.read_model(src), gf.read_model(dst)
    assert b.ftype == gf.FTYPE_Q4_0 and b.raw[gf.REL_BIAS_NAME] == a.raw[gf.REL_BIAS_NAME] and b.raw[gf.REL_BIAS_NAME][0] == gf.FTYPE_F16
    assert pybert.model_digest(dst)[0] == len(a.raw)
    m = pybert.BertModel(dst, tokenizer_only=True)
    assert m.relative_attention
    m.close()


def test_one_seed_one_encoder():
    a = gf.synthetic_weights(TINY, 5, n_labels=2, mlm_head=True)
    b = gf.synthetic_weights(TINY, 5, n_labels=2, mlm_head=True, rel_bias=True)
    assert set(b) - set(a) == {gf.REL_BIAS_NAME} and all(np.array_equal(a[k], b[k]) for k in a)
    assert b[gf.REL_BIAS_NAME].shape == (32, TINY.n_head) and 1.0 < b[gf.REL_BIAS_NAME].std() < 3.0


# ------------------------------------------------------------------------------------------------
# the tokenizer
# ------------------------------------------------------------------------------------------------
def _mpnet_vocab(n, with_sep=True):
    vocab = [f"[unused{i}]".encode() for i in range(n)]
    vocab[0], vocab[1], vocab[3] = b"<s>", b"<pad>", b"<unk>"
    if with_sep:
        vocab[2] = b"</s>"
    vocab[10], vocab[11], vocab[12] = b"hello", b"world", b"##s"
    return vocab


def test_texts_are_wrapped_in_the_files_own_ids(tmp_path):
    hp = dataclasses.replace(TINY, n_vocab=128)
    vocab = _mpnet_vocab(hp.n_vocab)
    bias = pybert.BertModel(_write(tmp_path / "bias.bin", hp, vocab=vocab), tokenizer_only=True)
    plain = pybert.BertModel(_write(tmp_path / "plain.bin", hp, rel_bias=False, vocab=vocab), tokenizer_only=True)
    assert bias.tokenize("hello worlds") == [0, 10, 11, 12, 2]
    assert plain.tokenize("hello worlds") == [101, 10, 11, 12, 102]          # a BERT file keeps 101 / 102 whatever its vocabulary holds
    assert bias.tokenize("") == [0, 2]
    assert bias.tokenize("hello " * 100, 8) == [0] + [10] * 6 + [2]         # truncation keeps room for </s>
    bias.close(); plain.close()


def test_a_vocabulary_without_the_closing_id_fails_the_load(tmp_path, capfd):
    hp = dataclasses.replace(TINY, n_vocab=128)
    path = _write(tmp_path / "nosep.bin", hp, vocab=_mpnet_vocab(hp.n_vocab, with_sep=False))
    with pytest.raises(RuntimeError):
        pybert.BertModel(path, tokenizer_only=True)
    assert "</s>" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    L, T = pybert.lib(), pybert.test_lib()
    assert "bert_hip_relative_attention" in pybert.BERT_HIP_H_SYMBOLS and hasattr(L, "bert_hip_relative_attention")
    for sym in ("bert_hip_test_attention_bias", "bert_hip_test_f32_attention_bias", "bert_hip_test_rel_bias_table"):
        assert sym in pybert.BERT_HIP_TEST_H_SYMBOLS and hasattr(T, sym) and not hasattr(L, sym)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bert_hip.h")).read()
    assert "bert_hip_relative_attention(struct bert_ctx *ctx)" in hdr
    for sym in pybert.BERT_HIP_H_SYMBOLS + pybert.BERT_HIP_TEST_H_SYMBOLS:
        if "relative" in sym or "bias" in sym:
            assert "token_index" not in sym and "hybrid" not in sym


def test_without_a_context_or_arguments():
    assert pybert.lib().bert_hip_relative_attention(None) == -1
    T = pybert.test_lib()
    out = np.zeros(3, dtype=np.float32)
    W = np.zeros((32, 1), dtype=np.float32)
    assert T.bert_hip_test_rel_bias_table(None, 1, 2, out.ctypes.data) == -1
    assert T.bert_hip_test_rel_bias_table(W.ctypes.data, 0, 2, out.ctypes.data) == -1
    assert T.bert_hip_test_rel_bias_table(W.ctypes.data, 1, 0, out.ctypes.data) == -1
    assert T.bert_hip_test_rel_bias_table(W.ctypes.data, 1, 2, out.ctypes.data) == 0
