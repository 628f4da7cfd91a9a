"""model_kernel.hip on full windows passes the residual x from one layer's tail to the next one's in lane order through a scratch
workspace: LayerNorm 2's result fragments as they are, no row-major rows between the layers.  Layer 0 reads the embedding kernel's rows,
the last layer writes rows for the pooling, the layers between neither read nor write rows.  Every comparison is bit equality against two
launches per layer (one_launch=0), which pass rows: every layer schedule (1 layer: rows in, rows out; 2: no inner layer; 3: one; 4: two)
at H = 256 and 384 with one workgroup and with three; the non-default pooling modes (instantiations of their own); a q4_0 file expanded
at load; the poison check — with every half of the scratch a NaN (the "test_poison_xres" option of libbert_test.so's engine) a full-window
pass gives the embeddings it gave before, so every element it reads it has written in the same launch; and full, ragged (which leaves
the scratch alone), full with other ids on one context: what an earlier pass left in the scratch does not show."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from test_multi_device import _cu

# (n_vocab, n_max_tokens, n_embd, n_intermediate, n_head, n_layer)
_DIMS = {f"res-h{H}-l{L}": (1000, 128, H, 4 * H, H // 32, L) for H in (256, 384) for L in (1, 2, 3, 4)}


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


def _full(hp, B, seed):
    return gf.synthetic_token_ids(B, 128, hp.n_vocab, seed=seed).reshape(-1), (np.arange(B + 1) * 128).astype(np.int32)


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
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dims", sorted(_DIMS))
def test_every_layer_schedule_gives_the_two_launch_bits(make_model, dims, B):
    m, hp = _model(make_model, dims)
    ids, cu = _full(hp, B, 41 + B)
    got, want = _both_routes(m, ids, cu)
    assert got.shape == (B, hp.n_embd) and np.isfinite(want).all()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert np.array_equal(m.eval_packed(ids, cu), got)          # (and the same bits on a second call)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [("mean", "0"), ("cls", "1"), ("cls", "0")])
def test_pooling_modes_read_the_last_layers_rows(make_model, mode):
    m, hp = _model(make_model, "res-h384-l3")
    m.set_option("pooling", mode[0])
    m.set_option("normalize", mode[1])
    ids, cu = _full(hp, 3, 57)
    got, want = _both_routes(m, ids, cu)
    assert np.isfinite(want).all() and np.array_equal(got, want), float(np.abs(got - want).max())
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", ["res-h256-l3", "res-h384-l4"])
def test_every_scratch_element_read_was_written_in_the_same_launch(make_model, dims):
    m, hp = _model(make_model, dims, test_routes=True)
    ids, cu = _full(hp, 3, 93)
    got, want = _both_routes(m, ids, cu)                     # (leaves this batch's fragments, and the two-launch route's y, in the scratch)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    # every half of the scratch a NaN: a tail that loaded anything no tail before it had stored would carry the NaN into its rows
    m.set_option("test_poison_xres", "1")
    poisoned, names = _names_of(m, lambda: m.eval_packed(ids, cu))
    assert "model_kernel" in names, names
    assert np.array_equal(poisoned, want), float(np.nanmax(np.abs(poisoned - want)))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", ["res-h256-l3", "res-h384-l3"])
def test_stale_scratch_of_an_earlier_batch_does_not_show(make_model, dims):
    m, hp = _model(make_model, dims)
    B = 3
    ids_a, cu = _full(hp, B, 11)
    ids_b, _ = _full(hp, B, 12)
    assert not np.array_equal(ids_a, ids_b)
    lens = [128, 17, 90, 64, 64]
    ragged_cu = _cu(lens)
    ragged_ids = np.random.default_rng(8).integers(0, hp.n_vocab, size=int(ragged_cu[-1])).astype(np.int32)
    m.set_option("one_launch", "0")
    want_b, want_ragged = m.eval_packed(ids_b, cu), m.eval_packed(ragged_ids, ragged_cu)
    m.set_option("one_launch", "1")
    m.eval_packed(ids_a, cu)
    m.set_option("one_launch", "2")                          # (the one-launch kernel whatever the fill of the windows: its ragged form)
    ragged, names = _names_of(m, lambda: m.eval_packed(ragged_ids, ragged_cu))
    assert "model_kernel" in names and not {"qkv_attention2", "layer_tail"} & names, names
    m.set_option("one_launch", "1")
    got_b, names = _names_of(m, lambda: m.eval_packed(ids_b, cu))
    assert "model_kernel" in names, names
    m.close()
    fresh, _ = _model(make_model, dims)
    fresh.set_option("one_launch", "1")
    fresh_b = fresh.eval_packed(ids_b, cu)
    fresh.close()
    assert np.isfinite(want_b).all() and np.isfinite(want_ragged).all()
    assert np.array_equal(ragged, want_ragged), float(np.abs(ragged - want_ragged).max())
    assert np.array_equal(got_b, want_b), float(np.abs(got_b - want_b).max())
    assert np.array_equal(got_b, fresh_b), float(np.abs(got_b - fresh_b).max())


@pytest.mark.gpu
def test_q4_file_expanded_at_load(make_model):
    m, hp = _model(make_model, "res-h384-l3", "q4_0")
    ids, cu = _full(hp, 2, 5)
    got, want = _both_routes(m, ids, cu)
    assert np.isfinite(want).all() and np.array_equal(got, want), float(np.abs(got - want).max())
    m.close()
