"""bert_hip_index_kmeans (search.hip's kmeans_update_kernel behind the partition's assignment) and BertIndex.train_partition.

The tolerance of the one-iteration check is derived, not measured.  u = 2^-24, gamma(n) = n u / (1 - n u).  A list has c live
members x_1 .. x_c (the f32 rows get_rows returns; the float64 reference sums them with an error of order c 2^-53, ignored).
  - Element e of the sum: any order of adding c f32 terms gives |s^_e - S_e| <= gamma(c - 1) * sum_r |x_r,e| =: E_e.
  - The norm: the squares and their sum are DIM products and DIM - 1 additions in some order, so the computed sum of squares
    is |s^|^2 (1 + t) with |t| <= gamma(DIM); a correctly rounded sqrt gives n^ = |s^| (1 + e_n), |e_n| <= gamma(DIM) + 2 u.
  - The centroid is s^_e / n^ with one more rounding: (s^_e / |s^|) (1 + d) / (1 + e_n), |d| <= u, a relative factor within
    rho = (u + |e_n|) / (1 - |e_n|) of 1.
  - | |s^| - |S| | <= |E| (the norm of the vector of the E_e), so with m = |S| - |E| > 0:
    |s^_e / |s^| - S_e / |S|| <= E_e / m + |S_e| |E| / (m |S|), and the factor adds rho (|S_e| + E_e) / m.
tol_e is the sum of these three terms."""
import numpy as np
import pytest

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "i8"]
N, DIM, NL, LONG = 1500, 72, 12, 5
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def unit(x):
    return (x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-30)).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    """the shapes of test_gpu_search_probe.py: 600 rows near one direction, 900 over ten more, centroid 7 a copy of centroid 3"""
    rng = np.random.default_rng(78)
    dirs = unit(rng.standard_normal((NL, DIM)))
    dirs[7] = dirs[3]
    of = np.concatenate([np.full(600, LONG), rng.choice([d for d in range(NL) if d not in (LONG, 7)], 900)])
    rows = unit(dirs[of] + 0.06 * rng.standard_normal((N, DIM)))[rng.permutation(N)]
    rows[100:110] = rows[100]
    # (initial centroids off the directions, so that an iteration moves them)
    init = unit(dirs + 0.05 * rng.standard_normal((NL, DIM)))
    init[7] = init[3]
    return rows, init, unit(rng.standard_normal((9, DIM))), rng.choice(N, 100, replace=False).astype(np.int32)


@pytest.fixture(scope="module")
def indexes(model, data):
    """per dtype an index of the rows with 100 of them removed"""
    rows, _, _, gone = data
    out = {}
    for dtype in DTYPES:
        ix = model.index(dim=DIM, dtype=dtype)
        ix.add(rows)
        assert ix.remove(gone) == len(gone)
        out[dtype] = ix
    yield out
    for ix in out.values():
        ix.close()


def assign(model, centroids, rows):
    """the rule of bert_hip.h through public calls: a k = 1 search of an f32 index of the centroids; -1 goes to list 0"""
    cix = model.index(dim=DIM, dtype="f32")
    cix.add(centroids)
    lists = cix.search(rows, 1)[0][:, 0]
    cix.close()
    return np.where(lists < 0, 0, lists)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_iteration_is_assign_then_normalised_sum(model, indexes, data, dtype):
    _, init, _, gone = data
    ix = indexes[dtype]
    live = np.setdiff1d(np.arange(N), gone).astype(np.int32)
    assert np.array_equal(ix.live_ids(), live)
    rows = ix.get_rows(live)
    lists = assign(model, init, rows)
    got = ix.kmeans(NL, 1, init)
    x = rows.astype(np.float64)
    moved = 0
    for l in range(NL):
        mem = x[lists == l]
        c = len(mem)
        if c == 0:
            assert np.array_equal(got[l].view(np.int32), init[l].view(np.int32)), l       # kept, bit for bit
            continue
        S = mem.sum(axis=0)
        E = gamma(c - 1) * np.abs(mem).sum(axis=0)
        nS, nE = np.linalg.norm(S), np.linalg.norm(E)
        m = nS - nE
        assert m > 0
        e_n = gamma(DIM) + 2 * U
        rho = (U + e_n) / (1 - e_n)
        tol = E / m + np.abs(S) * nE / (m * nS) + rho * (np.abs(S) + E) / m
        err = np.abs(got[l].astype(np.float64) - S / nS)
        print(f"{dtype} list {l}: {c} members, max err {err.max():.3e}, min tol {tol.min():.3e}, worst err / tol {(err / tol).max():.3f}")
        assert (err <= tol).all(), (l, c, float((err / tol).max()))
        moved += int(not np.array_equal(got[l], init[l]))
    assert (lists == 7).sum() == 0 and (lists == LONG).sum() > 512 and moved >= 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_is_deterministic_and_leaves_the_index_alone(indexes, data, dtype):
    _, init, queries, _ = data
    ix = indexes[dtype]
    ix.partition(init)
    before = (len(ix), ix.n_live, ix.n_lists, ix.partition_lists(), ix.centroids(), ix.search(queries, 10), ix.search_probed(queries, 10, 2))
    a, b = ix.kmeans(NL, 5, init), ix.kmeans(NL, 5, init)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    c = init
    for _ in range(5):                                               # n_iter iterations are n_iter calls of one
        c = ix.kmeans(NL, 1, c)
    assert np.array_equal(a.view(np.int32), c.view(np.int32))
    after = (len(ix), ix.n_live, ix.n_lists, ix.partition_lists(), ix.centroids(), ix.search(queries, 10), ix.search_probed(queries, 10, 2))
    assert before[:3] == after[:3]
    assert np.array_equal(before[3], after[3]) and np.array_equal(before[4].view(np.int32), after[4].view(np.int32))
    for x, y in ((before[5], after[5]), (before[6], after[6])):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32))
    ix.partition(None)
    assert ix.n_lists == 0


def test_kmeans_rejects_bad_arguments(indexes, data, capfd):
    import ctypes as C
    _, init, _, _ = data
    ix = indexes["f16"]
    f32p = C.POINTER(C.c_float)
    for n_lists, n_iter, cents in ((0, 1, init), (65537, 1, init), (NL, 0, init), (NL, 1, np.where(np.arange(DIM) == 3, np.nan, init).astype(np.float32))):
        c = np.ascontiguousarray(cents, dtype=np.float32)
        keep = c.copy()
        capfd.readouterr()
        assert ix.lib.bert_hip_index_kmeans(ix.ix, n_lists, n_iter, c.ctypes.data_as(f32p)) == -2
        assert "bert_hip_index_kmeans" in capfd.readouterr().err
        assert np.array_equal(c.view(np.int32), keep.view(np.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_train_partition_does_not_lower_the_objective(model, indexes, data, dtype):
    """The objective is the mean over the live rows of the row's score against its own centroid, in float64.  A Lloyd step
    cannot lower it in exact arithmetic; the slack is what f32 can cost: the assignment compares f32 scores, each within
    gamma(DIM) |x| |c| of the exact one, so a row may take a list whose exact score is lower by at most twice that, and the
    update's centroid is within the tolerance of the test above of the exact one — bounded here by gamma(N) (1 + rho) per
    element, so by sqrt(DIM) times that against a row of norm |x|."""
    ix = indexes[dtype]
    live = ix.live_ids()
    rows = ix.get_rows(live)
    x = rows.astype(np.float64)
    init = ix.get_rows(np.random.default_rng(0).choice(live, NL, replace=False))
    lists0 = assign(model, init, rows)
    before = float(np.einsum("rd,rd->r", x, init.astype(np.float64)[lists0]).mean())
    cents = ix.train_partition(n_lists=NL, n_iter=10, seed=0)
    assert ix.n_lists == NL and np.array_equal(cents.view(np.int32), ix.centroids().view(np.int32))
    lists = ix.partition_lists()[live]
    assert np.array_equal(lists, assign(model, cents, rows))
    after = float(np.einsum("rd,rd->r", x, cents.astype(np.float64)[lists]).mean())
    xn = np.linalg.norm(x, axis=1).max()
    cn = max(np.linalg.norm(init.astype(np.float64), axis=1).max(), np.linalg.norm(cents.astype(np.float64), axis=1).max())
    slack = 2 * gamma(DIM) * xn * cn + np.sqrt(DIM) * 2 * gamma(N) * xn
    print(f"{dtype}: objective {before:.6f} -> {after:.6f}, slack {slack:.2e}")
    assert after >= before - slack
    ix.partition(None)
