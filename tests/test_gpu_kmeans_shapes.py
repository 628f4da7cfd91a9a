"""bert_hip_index_kmeans (search.hip's kmeans_update_kernel) beyond one shape: all four forms, dims 1, 64, 65, 257 and 2048 (one
element per lane, one lane over, more elements than threads, the most a lane can own), lists of exactly 1, 2, 3, 4 and 5 members
(fewer than, as many as and one more than the waves that share a list), an empty list and one of more than 600.

One iteration is checked against the normalised float64 sum of each list's stored rows with the bound derived at the top of
test_gpu_kmeans.py, taken with the case's own dim and member count:
    tol_e = E_e / m + |S_e| |E| / (m |S|) + rho (|S_e| + E_e) / m,    E_e = gamma(c - 1) sum_r |x_r,e|,  m = |S| - |E|,
    rho = (u + e_n) / (1 - e_n),  e_n = gamma(dim) + 2 u.
For b1 every element of every partial sum is an integer below 2^24, exact in f32 in any order: E = 0 there.  The members of a
list are known by construction (rows around their own direction, every row with its own centroid by a wide margin, asserted in
float64 here and through partition_lists on the GPU), and the stored rows are the NumPy restatement, not get_rows.

At dim 1 a row's list is decided by its sign alone, so at most two lists have members: three layouts, (1, 2), (3, 4) and
(5, 620) positive and negative rows, cover the same member counts."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import index_reference as ref                                        # noqa: E402
from index_reference import DTYPES, U, gamma, restate_rows           # noqa: E402

from bert_cpp_amd import pybert                                      # noqa: E402

gpu = pytest.mark.gpu

DIMS = [1, 64, 65, 257, 2048]
LENGTHS = [1, 2, 3, 4, 5, 0, 640, 30]                                # rows per list; list 5 is empty
N_GONE = 20                                                          # rows of the long list removed before the run


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def layouts(dim):
    """[(rows, of, init, gone)]: rows [N, dim], the list of each by construction, the initial centroids, the rows to remove"""
    rng = np.random.default_rng(600 + dim)
    out = []
    if dim == 1:
        init = np.array([[0.8], [0.5], [-0.8], [-0.5]], np.float32)  # positive rows: list 0, negative rows: list 2
        for pos, neg in ((1, 2), (3, 4), (5, 620)):
            of = np.repeat([0, 2], [pos, neg])[rng.permutation(pos + neg)]
            rows = (np.where(of == 0, 1, -1) * rng.uniform(0.5, 1.5, pos + neg)).astype(np.float32)[:, None]
            out.append((rows, of, init, np.zeros(0, np.int32)))
    else:
        # rows around sign-pattern directions, one element in twenty with its sign flipped, so that the b1 rows of a list
        # differ too; the initial centroids are other vectors around the same directions: a centroid that is wrongly kept
        # is not the expected one in any form
        dirs = ref.sign_centroids(rng, len(LENGTHS), dim)
        init = ref.rows_around(rng, dirs, np.arange(len(LENGTHS)))
        of = ref.lengths_layout(rng, LENGTHS)
        rows = ref.rows_around(rng, dirs, of)
        rows = np.where(rng.random(rows.shape) < 0.05, -rows, rows)
        gone = rng.choice(np.nonzero(of == 6)[0], N_GONE, replace=False).astype(np.int32)
        out.append((rows, of, init, gone))
    for case in out:
        for a in case:
            a.setflags(write=False)
    return out


def check_layout(dim):
    """on the CPU: in every stored form each row's best centroid in float64 is its own, by more than four tolerances over the
    runner-up, so the f32 assignment cannot differ"""
    for rows, of, init, gone in layouts(dim):
        c = init.astype(np.float64)
        for dtype in DTYPES:
            x = restate_rows(rows, dtype).astype(np.float64)
            ex, tl = x @ c.T, ref.TOL * (np.abs(x) @ np.abs(c).T)
            assert np.array_equal(ex.argmax(axis=1), of), (dim, dtype)
            own = ex[np.arange(len(x)), of]
            ex[np.arange(len(x)), of] = -np.inf
            assert (own - ex.max(axis=1) > 4 * tl.max(axis=1)).all(), (dim, dtype)
        assert (of[gone] == 6).all()


def tolerance(mem, dim, exact_sums):
    """mem [c, dim] float64 -> (the exact centroid S / |S|, tol per element)"""
    c = len(mem)
    S = mem.sum(axis=0)
    E = np.zeros(dim) if exact_sums else gamma(c - 1) * np.abs(mem).sum(axis=0)
    nS, nE = np.linalg.norm(S), np.linalg.norm(E)
    m = nS - nE
    assert m > 0
    e_n = gamma(dim) + 2 * U
    rho = (U + e_n) / (1 - e_n)
    return S / nS, E / m + np.abs(S) * nE / (m * nS) + rho * (np.abs(S) + E) / m


def make_index(model, dim, dtype, rows, gone):
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    if len(gone):
        assert ix.remove(gone) == len(gone)
    return ix


@gpu
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_iteration_at_every_dim_and_list_length(model, dtype, dim):
    check_layout(dim)
    worst = (0.0, 0)
    counts = set()
    for rows, of, init, gone in layouts(dim):
        ix = make_index(model, dim, dtype, rows, gone)
        ix.partition(init)
        assert np.array_equal(ix.partition_lists(), of)
        ix.partition(None)
        got = ix.kmeans(len(init), 1, init)
        assert np.array_equal(got.view(np.int32), ix.kmeans(len(init), 1, init).view(np.int32))     # two runs, equal bits
        live = np.ones(len(rows), bool)
        live[gone] = False
        x = restate_rows(rows, dtype).astype(np.float64)
        for l in range(len(init)):
            mem = x[live & (of == l)]
            counts.add(len(mem))
            if len(mem) == 0:
                assert np.array_equal(got[l].view(np.int32), init[l].view(np.int32)), (dtype, dim, l)   # kept, bit for bit
                continue
            want, tol = tolerance(mem, dim, dtype == "b1")
            err = np.abs(got[l].astype(np.float64) - want)
            # (b1: an element whose exact sum is 0 has tolerance 0, and must be exactly 0)
            assert (err[tol == 0] == 0).all(), (dtype, dim, l, len(mem))
            ratio = float((err[tol > 0] / tol[tol > 0]).max())
            worst = max(worst, (ratio, len(mem)))
            assert (err <= tol).all(), (dtype, dim, l, len(mem), ratio)
        ix.close()
    print(f"kmeans {dtype} dim {dim}: worst err / tol {worst[0]:.3f} (a list of {worst[1]} members)")
    assert {0, 1, 2, 3, 4, 5} <= counts and max(counts) > 600


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_a_list_whose_members_cancel_keeps_its_centroid(model, dim):
    """f32 form: x and -x sum to exactly zero in any order, and a zero norm leaves the centroid as it is.  Beyond dim 1 the
    pairs are orthogonal to both centroids (every score +-0: the tie goes to list 0) and list 1 has ordinary members."""
    rng = np.random.default_rng(70 + dim)
    if dim == 1:
        init = np.array([[0.7]], np.float32)
        rows = np.array([[0.5], [-0.5], [1.25], [-1.25], [0.5], [-0.5]], np.float32)
        of = np.zeros(6, int)
    else:
        init = np.concatenate([ref.sign_centroids(rng, 2, dim - 1), np.zeros((2, 1), np.float32)], axis=1)
        pair = np.zeros((3, dim), np.float32)
        pair[:, -1] = [0.5, 1.0, 0.5]
        rows = np.concatenate([np.stack([pair, -pair], axis=1).reshape(6, dim), ref.rows_around(rng, init, np.ones(9, int))])
        of = np.repeat([0, 1], [6, 9])
        assert np.array_equal((rows.astype(np.float64) @ init.astype(np.float64).T).argmax(axis=1), of)
    ix = model.index(dim=dim, dtype="f32")
    ix.add(rows)
    ix.partition(init)
    assert np.array_equal(ix.partition_lists(), of)
    got = ix.kmeans(len(init), 1, init)
    assert np.array_equal(got[0].view(np.int32), init[0].view(np.int32))
    if dim > 1:
        want, tol = tolerance(rows[of == 1].astype(np.float64), dim, False)
        assert (np.abs(got[1].astype(np.float64) - want) <= tol).all() and not np.array_equal(got[1], init[1])
    ix.close()


@gpu
@pytest.mark.parametrize("dim", DIMS)
def test_an_i8_list_that_holds_a_nan_row_keeps_its_centroid(model, dim):
    """a row with an inf is stored as NaN, scores NaN against every centroid and so belongs to list 0, whose sum and norm are
    NaN: centroid 0 stays, bit for bit; the other lists — the same members at the same positions — move as without the row"""
    rows, of, init, gone = layouts(dim)[0]
    bad = np.ones((1, dim), np.float32)
    bad[0, dim // 2] = np.inf
    plain = make_index(model, dim, "i8", rows, gone)
    holed = make_index(model, dim, "i8", np.concatenate([rows, bad]), gone)
    assert np.isnan(holed.get_rows([len(rows)])).all()
    holed.partition(init)
    assert np.array_equal(holed.partition_lists(), np.concatenate([of, [0]]))
    a, b = plain.kmeans(len(init), 1, init), holed.kmeans(len(init), 1, init)
    assert (of == 0).sum() >= 1 and not np.array_equal(a[0], init[0])
    assert np.array_equal(b[0].view(np.int32), init[0].view(np.int32))
    assert np.array_equal(b[1:].view(np.int32), a[1:].view(np.int32))
    plain.close()
    holed.close()


# ---- without a GPU

@pytest.mark.parametrize("dim", DIMS)
def test_layouts_hold_in_float64(dim):
    check_layout(dim)
    for rows, of, init, gone in layouts(dim):
        if dim > 1:
            live = np.ones(len(rows), bool)
            live[gone] = False
            assert np.bincount(of[live], minlength=len(LENGTHS)).tolist() == [1, 2, 3, 4, 5, 0, 640 - N_GONE, 30]


def test_the_bound_holds_for_an_f32_sum_in_another_order():
    """the derived tolerance against a plain float32 restatement of the update (sequential sums, float32 norm and division):
    not the kernel's order, but an order the bound covers as well"""
    for dim in DIMS[1:]:
        rows, of, init, gone = layouts(dim)[0]
        for l in (3, 6):
            mem = rows[of == l]
            s = np.zeros(dim, np.float32)
            for r in mem:
                s = s + r
            n = np.sqrt(np.cumsum((s * s).astype(np.float32), dtype=np.float32)[-1])
            want, tol = tolerance(mem.astype(np.float64), dim, False)
            assert (np.abs((s / n).astype(np.float64) - want) <= tol).all()
