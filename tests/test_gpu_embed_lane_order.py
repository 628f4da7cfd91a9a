"""The one-launch route on full windows starts from the embedding in LANE ORDER: embed_ln_lanes_kernel (misc_kernels.hip) writes the
hidden state as model_kernel's layer 0 wants it, in the workspace the residual crosses through, and no rows; tail 0 and window phase 0
load it like every other layer's (layer_tail.hip's XRES layout, restated in lane_order.py).  Every comparison is bit equality.
Op level: bert_hip_test_embed_ln_lanes, put back into rows, against bert_hip_test_embed_ln on the same arguments.  End to end:
one_launch=1 against one_launch=0 (two launches per layer, rows all the way), with every workspace a NaN before the pass, with other
batches in between on one context, and for a batch that has the full shape only by the sum of its lengths."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import lane_order
from hip_graph import Hip
from test_gpu_parity import WT, _weight_bytes
from test_multi_device import _cu

pytestmark = pytest.mark.gpu

NAN16, NAN32 = 0x7E00, 0x7FC00000

# (n_vocab, n_max_tokens, n_embd, n_intermediate, n_head, n_layer): test_gpu_model_residual.py's geometries
_DIMS = {f"res-h{H}-l{L}": (1000, 128, H, 4 * H, H // 32, L) for H in (256, 384) for L in (1, 2, 3)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _same_bits(a, b, what):
    neq = np.argwhere(_bits(a) != _bits(b))
    assert len(neq) == 0, (what, len(neq), neq[:8].tolist())


# ------------------------------------------------------------------------------------------------
# 1. the kernel on its own
# ------------------------------------------------------------------------------------------------
def _tables(ftype, H, n_vocab, n_pos):
    rng = np.random.default_rng(11 * H + n_vocab + n_pos)
    tabs = [rng.normal(0, 1, (n, H)).astype(np.float32) for n in (n_vocab, 2, n_pos)]
    tabs[1][1] += 100.0                                  # (type row 1 is not used)
    tabs[2] += np.linspace(-2, 2, n_pos)[:, None].astype(np.float32)
    return [_weight_bytes(t, ftype)[0] for t in tabs]


def _ln_params(H):
    rng = np.random.default_rng(H)
    return (1 + rng.normal(0, 0.1, H)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)


# T = 128: two sentences inside one 128-token block (bisection); 256: two full sentences (position = t % 128); 384: full by the sum
# only -- blocks 0 and 1 bisect, block 2 is sentence 2 itself -- with a sentence longer than a block
LANE_BATCHES = [[60, 68], [128, 128], [127, 129, 128]]


@pytest.mark.parametrize("H", [256, 384])
@pytest.mark.parametrize("ftype", ["f32", "f16", "q4_0", "q4_1"])
def test_lane_order_embedding_is_the_rows_kernels_bits(ftype, H):
    """T = 128, 256 and 384 with the ids -1 and n_vocab among the tokens, zeros and quiet NaNs as the pad pattern: the un-permuted
    output equals the rows kernel's in every bit, no NaN is left inside [T][H] (every token was written) and the entry finds its
    pattern behind T (-4 otherwise, which raises)."""
    n_vocab, n_pos = 300, 160
    byts = _tables(ftype, H, n_vocab, n_pos)
    g, b = _ln_params(H)
    for lens in LANE_BATCHES:
        T = sum(lens)
        toks = np.random.default_rng(T + H).integers(0, n_vocab, size=T).astype(np.int32)
        toks[[0, 5, T // 2, T - 1]] = [-1, n_vocab, n_vocab, -1]
        rows = pybert.test_embed_ln(WT[ftype], *byts, H, g, b, toks, _cu(lens))
        lanes = pybert.test_embed_ln_lanes(WT[ftype], *byts, H, g, b, toks, _cu(lens))
        assert lanes is not None and lanes.shape == (T, H)
        _same_bits(lane_order.to_rows(lanes), rows, (ftype, H, lens))
        with pybert.test_pad(NAN16, NAN32):
            poisoned = pybert.test_embed_ln_lanes(WT[ftype], *byts, H, g, b, toks, _cu(lens))
        assert not np.isnan(poisoned).any(), ("the pad pattern is left inside [T][H]", ftype, H, lens)
        _same_bits(poisoned, lanes, ("NaN pad", ftype, H, lens))
        clamped = pybert.test_embed_ln_lanes(WT[ftype], *byts, H, g, b, np.clip(toks, 0, n_vocab - 1), _cu(lens))
        _same_bits(clamped, lanes, "ids -1 and n_vocab are ids 0 and n_vocab - 1")


@pytest.mark.parametrize("H", [256, 384])
def test_no_position_row_at_or_behind_max_len_is_read(H):
    """A position table of 160 rows whose rows from max_len = 128 on are NaN, lengths (127, 129, 128): every token is finite -- the
    offender's 129th takes row 127 -- and every token the rows kernel writes (its grid stops at place 127) has the rows kernel's bits."""
    n_vocab, n_pos, max_len = 300, 160, 128
    rng = np.random.default_rng(3 * H)
    word, typ = (rng.normal(0, 1, (n, H)).astype(np.float16) for n in (n_vocab, 2))
    pos = (rng.normal(0, 1, (n_pos, H)) + np.linspace(-2, 2, n_pos)[:, None]).astype(np.float16)
    pos[max_len:] = np.nan
    byts = [t.view(np.uint8).reshape(-1) for t in (word, typ, pos)]
    g, b = _ln_params(H)
    lens = [127, 129, 128]
    cu = _cu(lens)
    toks = rng.integers(0, n_vocab, size=int(cu[-1])).astype(np.int32)
    lanes = pybert.test_embed_ln_lanes(1, *byts, H, g, b, toks, cu, max_len)
    assert lanes is not None
    got = lane_order.to_rows(lanes)
    assert np.isfinite(got).all(), ("a position row at or behind max_len was read", np.argwhere(~np.isfinite(got))[:4].tolist())
    with pybert.test_pad(NAN16, NAN32):
        rows = pybert.test_embed_ln(1, *byts, H, g, b, toks, cu, max_len)
    written = np.ones(len(toks), dtype=bool)
    written[127 + 128] = False                            # (place 128 of sentence 1: behind the rows kernel's grid)
    assert np.isnan(rows[~written]).all() and np.isfinite(rows[written]).all()
    _same_bits(got[written], rows[written], "the tokens both kernels write")


@pytest.mark.parametrize("case", [("T 96", 384, [96]), ("T 130", 384, [130]), ("H 128", 128, [128])])
def test_shapes_the_launcher_declines(case):
    """T no multiple of 128, a width model_kernel does not have: the launcher returns false and launches nothing (the entry's -2)."""
    _, H, lens = case
    byts = _tables("f16", H, 50, 140)
    g, b = _ln_params(H)
    toks = np.arange(sum(lens), dtype=np.int32) % 50
    assert pybert.test_embed_ln_lanes(1, *byts, H, g, b, toks, _cu(lens)) is None
    assert pybert.test_embed_ln(1, *byts, H, g, b, toks, _cu(lens)).shape == (sum(lens), H)      # (the rows form takes it)


# ------------------------------------------------------------------------------------------------
# 2. end to end
# ------------------------------------------------------------------------------------------------
def _model(make_model, dims, test_routes=False):
    gf.MODEL_DIMS.setdefault(dims, gf.BertHParams(*_DIMS[dims]))
    path, hp = make_model(dims, "f16", 0)
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


@pytest.mark.parametrize("dims", sorted(_DIMS))
def test_one_launch_from_lane_order_gives_the_two_launch_bits(make_model, dims):
    """B = 1, 2 and 5 full sentences: the one-launch pass is two kernels, embed_ln and model_kernel, and gives the bits of two launches
    per layer; the same once more with every workspace of the engine a NaN before the pass (x, y and the rest: whatever layer 0 reads,
    this pass's embedding kernel wrote)."""
    m, hp = _model(make_model, dims, test_routes=True)
    for B in (1, 2, 5):
        ids, cu = _full(hp, B, 70 + B)
        m.set_option("one_launch", "0")
        want, names = _names_of(m, lambda: m.eval_packed(ids, cu))
        assert {"qkv_attention2", "layer_tail"} <= names and "model_kernel" not in names, names
        m.set_option("one_launch", "1")
        got, names = _names_of(m, lambda: m.eval_packed(ids, cu))
        assert names == {"embed_ln", "model_kernel"}, names
        assert got.shape == (B, hp.n_embd) and np.isfinite(want).all()
        assert np.array_equal(got, want), (B, float(np.abs(got - want).max()))
        m.set_option("test_poison_workspace", "1")
        poisoned, names = _names_of(m, lambda: m.eval_packed(ids, cu))
        assert names == {"embed_ln", "model_kernel"}, names
        assert np.array_equal(poisoned, want), (B, "poisoned", float(np.nanmax(np.abs(poisoned - want))))
    m.close()


@pytest.mark.parametrize("dims", ["res-h256-l2", "res-h384-l3"])
def test_full_ragged_full_on_one_context(make_model, dims):
    """A full batch, a ragged one through the one-launch kernel's ragged form (rows from the rows kernel), a full one with other ids:
    each as a fresh context computes it -- neither embedding form leaves anything the other route's pass reads."""
    m, hp = _model(make_model, dims)
    ids_a, cu = _full(hp, 3, 21)
    ids_b, _ = _full(hp, 3, 22)
    ragged_cu = _cu([128, 17, 90, 64, 85])                  # (384 tokens as well: T alone does not pick the form)
    ragged_ids = np.random.default_rng(9).integers(0, hp.n_vocab, size=int(ragged_cu[-1])).astype(np.int32)
    m.set_option("one_launch", "1")
    got_a = m.eval_packed(ids_a, cu)
    m.set_option("one_launch", "2")
    got_r, names = _names_of(m, lambda: m.eval_packed(ragged_ids, ragged_cu))
    assert "model_kernel" in names and not {"qkv_attention2", "layer_tail"} & names, names
    m.set_option("one_launch", "1")
    got_b, names = _names_of(m, lambda: m.eval_packed(ids_b, cu))
    assert names == {"embed_ln", "model_kernel"}, names
    m.close()
    for got, ids, c, opt in ((got_a, ids_a, cu, "1"), (got_r, ragged_ids, ragged_cu, "2"), (got_b, ids_b, cu, "1")):
        for route in (opt, "0"):
            fresh, _ = _model(make_model, dims)
            fresh.set_option("one_launch", route)
            want = fresh.eval_packed(ids, c)
            fresh.close()
            assert np.isfinite(want).all() and np.array_equal(got, want), (opt, route, float(np.abs(got - want).max()))


@pytest.mark.parametrize("dims", ["res-h256-l2", "res-h384-l2"])
def test_full_shape_by_the_sum_of_the_lengths_only(make_model, dims):
    """Lengths (127, 129, 128) under a promised max_len of 128 through the device entry: T = 3 x 128, so the pass takes the full-window
    form, whose blocks 0 and 1 are no sentences.  As before the lane-order embedding (recorded on the commit before it, same output):
    the status word is set, rows 0 and 1 are NaN -- the pooling guard's, for a sentence that is not its block -- and row 2, whose block
    is the sentence, has the bits of that sentence evaluated alone.  (The embedding kernel finds sentence and position of blocks 0 and 1
    by bisection, clamps the offender's place 128 to position row 127, and reads no token behind T = 384: its grid is T / 32 blocks.)"""
    m, hp = _model(make_model, dims)
    hip = Hip()
    lens = [127, 129, 128]
    cu = _cu(lens)
    T, B, H = int(cu[-1]), 3, hp.n_embd
    toks = np.random.default_rng(31).integers(0, hp.n_vocab, size=T).astype(np.int32)
    m.set_option("one_launch", "1")
    alone = m.eval_packed(toks[cu[2]:], _cu([128]))
    assert m.check() == 0
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.upload(np.full((B, H), 7.0, np.float32))
    m.reserve(T, B)
    _, names = _names_of(m, lambda: m.eval_packed_device(d_t, d_cu, B, T, 128, d_out, 0))
    got = hip.download(d_out, (B, H))
    status = m.check()
    print(f"LANESUM {dims}: status {status}, NaN rows {np.isnan(got).all(axis=1).tolist()}, row 2 equal {bool(np.array_equal(got[2], alone[0]))}")
    assert names == {"embed_ln", "model_kernel"}, names
    assert status != 0
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
    assert np.isfinite(alone).all() and np.array_equal(got[2], alone[0])
    hip.free(d_t, d_cu, d_out)
    m.close()
