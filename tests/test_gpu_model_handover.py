"""model_kernel.hip on full windows hands the hidden state from a layer's LayerNorm 2 to the next layer's Q|K|V projection in
registers (the same waves, lanes and tokens; a lane-half exchange per fragment) and its window phases take slot -> token from the
window's index alone.  What test_gpu_parity's equal-bits test (six layers, H = 384) does not pin: H = 256, models of one and two
layers (the peeled first window phase alone; the first hand-over alone), and a batch that has the full-window shape only by the
sum of its lengths.  Every comparison is bit equality against two launches per layer (one_launch=0), which loads x from memory."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from test_multi_device import _Hip, _cu

# (n_vocab, n_max_tokens, n_embd, n_intermediate, n_head, n_layer)
_DIMS = {"h256-l1": (1000, 128, 256, 1024, 8, 1), "h256-l2": (1000, 128, 256, 1024, 8, 2), "h256-l3": (1000, 128, 256, 1024, 8, 3),
         "h384-l1": (1000, 128, 384, 1536, 12, 1), "h384-l2": (1000, 128, 384, 1536, 12, 2)}


def _register(dims):
    gf.MODEL_DIMS.setdefault(dims, gf.BertHParams(*_DIMS[dims]))


def _names_of(m, run):
    m.profile(True)
    got = run()
    names = set(m.profile_report())
    m.profile(False)
    return got, names


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("dims", sorted(_DIMS))
def test_full_windows_in_one_launch_give_the_two_launch_bits(make_model, dims, B):
    _register(dims)
    path, hp = make_model(dims, "f16", 0)
    m = pybert.BertModel(path)
    m.set_option("latency", "0")
    ids = gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=11 + B)
    cu = (np.arange(B + 1) * 128).astype(np.int32)
    got, names = _names_of(m, lambda: m.eval_packed(ids.reshape(-1), cu))
    assert names == {"embed_ln", "model_kernel"}, names
    m.set_option("one_launch", "0")
    want, names = _names_of(m, lambda: m.eval_packed(ids.reshape(-1), cu))
    assert {"qkv_attention2", "layer_tail"} <= names and "model_kernel" not in names, names
    assert np.isfinite(want).all() and got.shape == (B, hp.n_embd)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    m.set_option("one_launch", "1")
    again = m.eval_packed(ids.reshape(-1), cu)               # (and the same bits every time)
    assert np.array_equal(again, got)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", ["h256-l2", "minilm-l6"])
def test_a_batch_that_is_full_only_by_its_sum(make_model, dims, capfd):
    """T = 128 B and max_len = 128 promised, but one sentence is long and the next one short (twice): the full-window form works
    128-token block by block.  The sentences that are not exactly their block — the offenders — get a NaN row and the status word;
    every sentence whose block holds no offender keeps the two-launch route's bits.  (The rows of x inside an offender's block
    are not meaningful and not looked at.)"""
    if dims in _DIMS:
        _register(dims)
    hip = _Hip()
    path, hp = make_model(dims, "f16", 0)
    m = pybert.BertModel(path)
    m.set_option("latency", "0")
    lens = [128, 128, 200, 56, 128, 128, 100, 156, 128]
    clean, offenders = [0, 1, 4, 5, 8], [2, 3, 6, 7]
    cu = _cu(lens)
    T, B, H = int(cu[-1]), len(lens), hp.n_embd
    assert T == 128 * B
    for b in range(B):
        assert (b in clean) == (int(cu[b]) == 128 * b and lens[b] == 128)
    toks = np.random.default_rng(4).integers(0, hp.n_vocab, size=T).astype(np.int32)
    m.set_option("one_launch", "0")
    cu_clean = (np.arange(len(clean) + 1) * 128).astype(np.int32)
    want, names = _names_of(m, lambda: m.eval_packed(np.concatenate([toks[cu[b]:cu[b + 1]] for b in clean]), cu_clean))
    assert {"qkv_attention2", "layer_tail"} <= names and "model_kernel" not in names, names
    m.set_option("one_launch", "1")
    out = hip.upload(np.full((B, H), 7.0, np.float32))
    d_t, d_cu = hip.upload(toks), hip.upload(cu)
    m.reserve(T, B)
    _, names = _names_of(m, lambda: m.eval_packed_device(d_t, d_cu, B, T, 128, out, 0))
    got = hip.download(out, (B, H))
    assert "model_kernel" in names and not {"qkv_attention2", "layer_tail"} & names, names
    assert m.check() == 1 and m.check() == 0
    for b in offenders:
        assert np.isnan(got[b]).all(), b
    assert np.isfinite(got[clean]).all()
    assert np.array_equal(got[clean], want), float(np.abs(got[clean] - want).max())
    capfd.readouterr()
    m.close()
