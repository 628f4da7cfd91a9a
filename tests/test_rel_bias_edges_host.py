"""What test_gpu_rel_bias_edges.py rests on, checked without a GPU: the table staging of attention_mfma_kernel restated in NumPy against
rel_bias_reference.bias_matrix for every (sentence length, table length) the GPU tests use; that the float64 references and the derived
bounds can tell a kernel with a wrong lookup (key - query negated, the distance off by one) on the inputs of every op-level case; and the
walk geometry the moving-table test asserts of itself on the device, from the grid rule restated for 256 compute units."""
import numpy as np
import pytest

import rel_bias_reference as rb
from attention_walk import persistent_grid, walk_lengths
from test_gpu_launch_geometry import WALK_LENS

N_HEAD = 2


# ------------------------------------------------------------------------------------------------
# the staging
# ------------------------------------------------------------------------------------------------
def staged_bias(rel, h, n, P, staged=None):
    """attention_mfma_kernel's lookup: the window tbl[i] = rel[h][P - n + i], i < 2 n - 1, and the score of (query q, key) starts from
    tbl[key - q + n - 1].  staged: only the first `staged` entries are written (a staging loop that is cut short); the rest keeps what
    the slots held, here a value no table has."""
    tbl = np.full(2 * n - 1, 1e30)
    m = 2 * n - 1 if staged is None else min(staged, 2 * n - 1)
    tbl[:m] = rel[h][P - n:P - n + m]
    q = np.arange(n)
    return tbl[q[None, :] - q[:, None] + n - 1]


def _pairs():
    """every (sentence length, table length) of the GPU tests"""
    pairs = {(n, rb.P_LONG) for n in rb.LONG_LENS + (129,)}
    pairs |= {(n, P) for P, lens in rb.MOVING_WALK.values() for n in lens}
    pairs |= {(n, 512) for n in tuple(WALK_LENS) + rb.LENS + rb.GENERIC_LENS + (2,)}
    pairs |= {(n, 512) for lens in rb.HARD_CASES.values() for n in lens}
    pairs |= {(n, P) for lens, Ps in rb.P_FREE.values() for n in lens for P in Ps}
    pairs |= {(n, 128) for n in rb.P_SMALL_LENS} | {(1152, 1152), (512, 512)}
    pairs |= {(n, hp.n_max_tokens) for hp, _, calls in rb.E2E_EDGE_MODELS.values() for c in calls for n in c}
    assert all(n <= P for n, P in pairs)
    return sorted(pairs)


def test_the_staged_window_is_the_bias_matrix():
    W = rb.draw_W(N_HEAD, seed=5)
    tables = {}
    for n, P in _pairs():
        rel = tables.setdefault(P, rb.rel_table(W, P))
        assert rel.shape == (N_HEAD, 2 * P - 1)
        for h in range(N_HEAD):
            assert np.array_equal(staged_bias(rel, h, n, P), rb.bias_matrix(W, h, n)), (n, P, h)


@pytest.mark.parametrize("n", [600, 1025, 1152])
def test_a_staging_without_its_strided_loop_differs(n):
    """512 threads prefetch two entries each: without the loop behind them entries 1024 .. 2 n - 2 are stale, and beyond 512 tokens
    some (query, key) pairs read them; up to 512 tokens none does"""
    W = rb.draw_W(N_HEAD, seed=5)
    rel = rb.rel_table(W, rb.P_LONG)
    short = staged_bias(rel, 0, n, rb.P_LONG, staged=1024)
    stale_pairs = sum(n - abs(i - (n - 1)) for i in range(1024, 2 * n - 1))                  # entry i serves the n - |i - (n - 1)| pairs of its diagonal
    assert stale_pairs > 0 and (short != rb.bias_matrix(W, 0, n)).sum() == stale_pairs
    assert np.array_equal(staged_bias(rel, 0, 512, rb.P_LONG, staged=1024), rb.bias_matrix(W, 0, 512))


# ------------------------------------------------------------------------------------------------
# the references can see a wrong kernel
# ------------------------------------------------------------------------------------------------
def _rows_outside(lens, n_head, d_head, kind, wrong, **kw):
    """per sentence (n, the number of rows in which the float64 result of the wrong lookup leaves the bound of the right one)"""
    _, _, want, bnd = rb.reference(lens, n_head, d_head, kind, **kw)
    _, _, other, _ = rb.reference(lens, n_head, d_head, kind, wrong=wrong, **kw)
    out = (np.abs(other - want) > bnd).any(axis=1)
    cu = rb.cu_of(lens)
    return [(n, int(out[cu[b]:cu[b + 1]].sum())) for b, n in enumerate(lens)]


def _every_row(per_sentence):
    return all(k == n for n, k in per_sentence if n >= 2)


# (what, lengths, d_heads, kernels): the op-level cases of test_gpu_rel_bias_edges.py under W ~ N(0, 2^2)
PLAIN_CASES = [
    ("long keys", rb.LONG_LENS, (32,), ("mfma",)),
    ("moving walk 32", rb.MOVING_WALK[32][1], (32,), ("mfma",)),
    ("moving walk 64", rb.MOVING_WALK[64][1], (64,), ("mfma",)),
    ("P one chunk", rb.P_FREE["one chunk"][0], (32, 64), ("mfma", "naive", "f32")),
    ("P persistent", rb.P_FREE["persistent"][0], (32, 64), ("mfma", "naive", "f32")),
    ("P 128", rb.P_SMALL_LENS, (32, 64), ("mfma", "naive", "f32")),
    ("alone", rb.LENS, (32, 64), ("mfma", "naive", "f32")),
    ("generic", rb.GENERIC_LENS, rb.GENERIC_D_HEADS, ("naive",)),
]


@pytest.mark.parametrize("what,lens,d_heads,kinds", PLAIN_CASES, ids=[c[0] for c in PLAIN_CASES])
def test_a_negated_distance_leaves_the_bound_in_every_row(what, lens, d_heads, kinds):
    for d_head in d_heads:
        for kind in kinds:
            per = _rows_outside(lens, N_HEAD, d_head, kind, "negated")
            assert _every_row(per), (what, d_head, kind, per)


@pytest.mark.parametrize("case", list(rb.HARD_CASES))
def test_hard_values_show_a_wrong_lookup(case):
    """negated: every row; off by one: every row where the score is the bias alone, at least half the rows where the maximum moves"""
    lens = rb.HARD_CASES[case]
    for d_head in (32, 64):
        for kind in ("mfma", "naive", "f32"):
            per = _rows_outside(lens, N_HEAD, d_head, kind, "negated", case=case)
            assert _every_row(per), (case, d_head, kind, "negated", per)
            per = _rows_outside(lens, N_HEAD, d_head, kind, "off_by_one", case=case)
            if case == "lookup":
                assert _every_row(per), (case, d_head, kind, "off by one", per)
            if case in ("rise", "fall"):
                assert all(2 * k >= n for n, k in per), (case, d_head, kind, "off by one", per)


@pytest.mark.parametrize("d_head", [32, 64])
def test_the_deep_walk_shows_a_negated_distance(d_head):
    """the deep walk's recipe at 256 compute units (65 sentences of WALK_LENS, 12 heads), every 16th item"""
    n_head, cus = 12, 256
    B = next(b for b in range(1, 4096) if b * n_head >= 3 * cus + 8 and (b * n_head) % 8)
    rng = np.random.default_rng(2000 * d_head + n_head)
    lens = tuple([512] + [int(n) for n in rng.choice(WALK_LENS, size=B - 1)])
    items = range(0, B * n_head, 16)
    qkv, W = rb.op_inputs(lens, n_head, d_head), rb.draw_W(n_head)
    want, bnd = rb.attention_packed(qkv, lens, n_head, d_head, W, "mfma", items=items)
    other, _ = rb.attention_packed(qkv, lens, n_head, d_head, W, "mfma", items=items, wrong="negated")
    cu = rb.cu_of(lens)
    for it in items:
        b, h = divmod(it, n_head)
        rows, sl = slice(cu[b], cu[b + 1]), slice(h * d_head, (h + 1) * d_head)
        out = (np.abs(other[rows, sl] - want[rows, sl]) > bnd[rows, sl]).any(axis=1)
        assert lens[b] < 2 or out.all(), (b, h, lens[b], int(out.sum()))


@pytest.mark.parametrize("kind", ["naive", "f32"])
def test_the_many_sentences_show_a_negated_distance(kind):
    qkv, W = rb.many_inputs(), rb.draw_W(1)
    want, bnd = rb.many_reference(qkv.astype(np.float32) if kind == "f32" else qkv, W, kind)
    other, _ = rb.many_reference(qkv.astype(np.float32) if kind == "f32" else qkv, W, kind, wrong="negated")
    out = (np.abs(other - want) > bnd).any(axis=1)
    assert out.all(), (int((~out).sum()), np.flatnonzero(~out)[:5].tolist())


def test_the_batched_bounds_are_the_bounds():
    """naive_bound and f32_bound over a leading axis of sentences = sentence by sentence"""
    rng = np.random.default_rng(2)
    q, k, v = (rng.normal(0, 1, (5, 9, 4)).astype(np.float16) for _ in range(3))
    b = rb.bias_matrix(rb.draw_W(1), 0, 9)
    for kind in ("naive", "f32"):
        bnd, want = rb.BOUNDS[kind](q, k, v, b)
        for s in range(5):
            b1, w1 = rb.BOUNDS[kind](q[s], k[s], v[s], b)
            assert np.array_equal(bnd[s], b1) and np.array_equal(want[s], w1), (kind, s)


# ------------------------------------------------------------------------------------------------
# the walk geometry of the moving-table test
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_head", [32, 64])
def test_the_moving_walk_moves(d_head):
    """what test_a_walk_moves_the_table asserts of its launch on the device, at 256 compute units"""
    P, lens = rb.MOVING_WALK[d_head]
    assert max(lens) <= P and max(lens) > 128
    items = len(lens) * N_HEAD
    grid = persistent_grid(items, cus=256)
    assert (items, grid) == (26, 24)
    walked = [w for w in walk_lengths(lens, N_HEAD, grid) if len(w) > 1]
    pads = [[(n + 127) // 128 for n in w] for w in walked]
    assert len(walked) >= 2 and any(p[1] > p[0] for p in pads) and any(p[1] < p[0] for p in pads)
    assert walked[0][0] == 512 and walked[0][1] == 5 and walked[1][0] == 7
    if d_head == 32:
        assert any(n > 1024 for w in walked for n in w[1:])
