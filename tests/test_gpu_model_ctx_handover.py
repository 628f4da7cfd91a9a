"""model_kernel.hip on full windows hands the attention context from the attention waves to the layer tail on chip: the tail's U waves
are the attention waves and keep the fragments in registers, the D waves get them through the dead weight ring in LDS, and no ctx is
stored or loaded.  Every comparison is bit equality against two launches per layer (one_launch=0), which stores and loads ctx:
H = 256 and 384; one layer (no rotated turn), two (one) and six; B = 1, 5, 130, 256; q4 files expanded at load; and a full batch,
a ragged one and a full one again on the same context (the ragged form still goes through the ctx workspace and must not see what
an earlier pass left there, the full form must not depend on it); and the poison check: with every half of the context's ctx workspace
a NaN (the "test_poison_ctx" option of libbert_test.so's engine) a full-window pass gives the same embeddings, so it reads none of it."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from test_multi_device import _cu

# (n_vocab, n_max_tokens, n_embd, n_intermediate, n_head, n_layer)
_DIMS = {"ctx-h256-l1": (1000, 128, 256, 1024, 8, 1), "ctx-h256-l2": (1000, 128, 256, 1024, 8, 2), "ctx-h256-l6": (1000, 128, 256, 1024, 8, 6),
         "ctx-h384-l1": (1000, 128, 384, 1536, 12, 1), "ctx-h384-l2": (1000, 128, 384, 1536, 12, 2), "ctx-h384-l6": (1000, 128, 384, 1536, 12, 6)}


def _model(make_model, dims, ftype="f16", test_routes=False):
    gf.MODEL_DIMS.setdefault(dims, gf.BertHParams(*_DIMS[dims]))
    path, hp = make_model(dims, ftype, 0)
    m = pybert.BertModel(path, test_routes=test_routes)
    m.set_option("latency", "0")
    return m, hp


def _names_of(m, run):
    m.profile(True)
    got = run()
    names = set(m.profile_report())
    m.profile(False)
    return got, names


def _both_routes(m, ids, cu):
    m.set_option("one_launch", "1")
    got, names = _names_of(m, lambda: m.eval_packed(ids, cu))
    assert "model_kernel" in names and not {"qkv_attention2", "layer_tail"} & names, names
    m.set_option("one_launch", "0")
    want, names = _names_of(m, lambda: m.eval_packed(ids, cu))
    assert {"qkv_attention2", "layer_tail"} <= names and "model_kernel" not in names, names
    m.set_option("one_launch", "1")
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 130, 256])
@pytest.mark.parametrize("dims", sorted(_DIMS))
def test_full_windows_without_a_stored_context_give_the_two_launch_bits(make_model, dims, B):
    m, hp = _model(make_model, dims)
    ids = gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=31 + B).reshape(-1)
    cu = (np.arange(B + 1) * 128).astype(np.int32)
    got, want = _both_routes(m, ids, cu)
    assert got.shape == (B, hp.n_embd) and np.isfinite(want).all()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert np.array_equal(m.eval_packed(ids, cu), got)          # (and the same bits every time)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ftype", ["q4_0", "q4_1"])
@pytest.mark.parametrize("dims", ["ctx-h256-l2", "ctx-h384-l6"])
def test_q4_files_expanded_at_load(make_model, dims, ftype):
    m, hp = _model(make_model, dims, ftype)
    B = 7
    ids = gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=5).reshape(-1)
    cu = (np.arange(B + 1) * 128).astype(np.int32)
    got, want = _both_routes(m, ids, cu)
    assert np.isfinite(want).all() and np.array_equal(got, want), float(np.abs(got - want).max())
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", ["ctx-h256-l2", "ctx-h384-l6"])
def test_full_then_ragged_then_full_on_one_context(make_model, dims):
    m, hp = _model(make_model, dims)
    B = 9
    full_ids = gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=77).reshape(-1)
    full_cu = (np.arange(B + 1) * 128).astype(np.int32)
    lens = [128, 17, 90, 128, 3, 64, 64, 101, 128]
    ragged_cu = _cu(lens)
    ragged_ids = np.random.default_rng(8).integers(0, hp.n_vocab, size=int(ragged_cu[-1])).astype(np.int32)
    m.set_option("one_launch", "0")
    want_full, want_ragged = m.eval_packed(full_ids, full_cu), m.eval_packed(ragged_ids, ragged_cu)
    m.set_option("one_launch", "1")
    first, names = _names_of(m, lambda: m.eval_packed(full_ids, full_cu))
    assert "model_kernel" in names, names
    m.set_option("one_launch", "2")                          # (the one-launch kernel whatever the fill of the windows)
    ragged, names = _names_of(m, lambda: m.eval_packed(ragged_ids, ragged_cu))
    assert "model_kernel" in names and not {"qkv_attention2", "layer_tail"} & names, names
    m.set_option("one_launch", "1")
    again = m.eval_packed(full_ids, full_cu)
    assert np.isfinite(want_full).all() and np.isfinite(want_ragged).all()
    assert np.array_equal(first, want_full), float(np.abs(first - want_full).max())
    assert np.array_equal(ragged, want_ragged), float(np.abs(ragged - want_ragged).max())
    assert np.array_equal(again, want_full), float(np.abs(again - want_full).max())
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("dims", ["ctx-h256-l1", "ctx-h256-l6", "ctx-h384-l2", "ctx-h384-l6"])
def test_full_windows_do_not_read_the_ctx_workspace(make_model, dims, B):
    m, hp = _model(make_model, dims, test_routes=True)
    ids = gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=91 + B).reshape(-1)
    cu = (np.arange(B + 1) * 128).astype(np.int32)
    got, want = _both_routes(m, ids, cu)                     # (the two-launch pass leaves this batch's ctx behind)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    # every half of ctx a NaN: a full-window pass that still loaded any of it would carry the NaN into its rows
    m.set_option("test_poison_ctx", "1")
    poisoned, names = _names_of(m, lambda: m.eval_packed(ids, cu))
    assert "model_kernel" in names, names
    assert np.array_equal(poisoned, want), float(np.nanmax(np.abs(poisoned - want)))
    m.close()
