"""get_rows, the cluster partition, the probed (IVF) search and the rescore beyond one shape: dims 1 to 2048, lists of 1, 31, 32,
33, 127, 128, 129 and 650 rows, k on both sides of the 256 / 512 queue lengths, up to 300 lists and 256 probes, tails on both
sides of the 1024-row chunk, and more queries than one internal chunk of 4096.

The references are NumPy, written in index_reference.py and independent of the kernels: get_rows bit for bit against the stored
form; i8 and b1 results bit for bit against the restated integer arithmetic; f32 and f16 results by the float64 rule of
test_gpu_search.py (2e-6 * sum |q_i r_i| per score) restricted to the permitted rows; the list of a row and the lists a query
probes by float64 rankings of the centroids, the latter only where the ranking is safe from f32 rounding, which the fixtures
assert on the CPU for every query (the unmarked tests below run them, and the references against each other, without a GPU).
Every probed or rescored result is also compared bit for bit with search(..., allow=the permitted rows): the documented
contract.  The fixtures are built once per shape and never written to."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import index_reference as ref                                        # noqa: E402
from index_reference import DTYPES, assert_same, restate_rows, unit  # noqa: E402

from bert_cpp_amd import pybert                                      # noqa: E402

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def randn(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


# ---- 1. get_rows and assignment

ROWS_DIMS = [1, 7, 130, 384, 768, 2048]
N_ROWS = 700


@functools.lru_cache(maxsize=None)
def rows_case(dim):
    """700 Gaussian rows, among them a row with negative zeros, a row with no element above zero and a row of zeros of both
    signs; 900 ids in random order with repeats; Gaussian centroids for 1, 33 (number 20 a copy of number 4: empty) and 1000
    lists"""
    rng = np.random.default_rng(1000 + dim)
    rows = randn(rng, N_ROWS, dim)
    rows[3, ::2] = -0.0
    rows[5] = -np.abs(rows[5])
    rows[6] = 0.0
    rows[6, ::3] = -0.0
    ids = rng.integers(0, N_ROWS, 900).astype(np.int32)
    cents = {n: randn(rng, n, dim) for n in (1, 33, 1000)}
    cents[33][20] = cents[33][4]
    frozen(rows, ids, *cents.values())
    return rows, ids, cents


@gpu
@pytest.mark.parametrize("dim", ROWS_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_get_rows_and_lists_at_every_dim(model, dtype, dim):
    rows, ids, cents = rows_case(dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    stored = restate_rows(rows, dtype)
    assert np.array_equal(ix.get_rows(ids).view(np.int32), stored[ids].view(np.int32))
    for n_lists, c in cents.items():
        ix.partition(c)
        assert ix.n_lists == n_lists
        lists = ix.partition_lists()
        ref.check_lists(lists, stored, c, (dtype, dim, n_lists))
        if n_lists == 33:
            assert not (lists == 20).any()                           # the copy loses every tie to list 4
    ix.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_of_65536_centroids(model, dtype):
    rows, _, _ = rows_case(7)
    cents = randn(np.random.default_rng(65536), 65536, 7)
    ix = model.index(dim=7, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    assert ix.n_lists == 65536
    lists = ix.partition_lists()
    ref.check_lists(lists, restate_rows(rows, dtype), cents, dtype)
    assert lists.max() > 256
    ix.close()


# ---- 2. the probed search grid

GRID_DIMS = [7, 130, 384, 768, 2048]
LENGTHS = [1, 31, 32, 33, 127, 128, 129, 0, 650, 40]                 # rows per list; list 7 is empty
NL = len(LENGTHS)
KS = [1, 127, 128, 129, 256]
NPROBES = [1, 2, NL]


@functools.lru_cache(maxsize=None)
def grid_case(dim):
    """rows whose lists have the lengths above by construction (index_reference.rows_around), shuffled; three more rows for
    the tail; per list a query that leans to its centroid — so every list, the one-row list and the empty one too, is some
    query's first probe — and four Gaussian queries.  The lean is min(2, 6 / sqrt(dim)) of the centroid on a unit Gaussian
    vector, whose score against another centroid is N(0, 1 / dim): six deviations, and no more.  A query that is all
    centroid has 2048 products of one sign with each row of its list, and on such a sum a correctly rounded f32 fma chain in
    the kernel's order (index_reference.f32_chain_scores) errs by up to 1.07 of the 2e-6 tolerance, which the project set on
    Gaussian data; test_f32_chain_meets_the_tolerance_on_the_grid_fixture holds the fixture to what that chain can meet."""
    rng = np.random.default_rng(2000 + dim)
    cents = ref.sign_centroids(rng, NL, dim)
    of = ref.lengths_layout(rng, LENGTHS)
    rows = ref.rows_around(rng, cents, of)
    tail = ref.rows_around(rng, cents, rng.integers(0, NL, 3))
    queries = unit(np.concatenate([min(2.0, 6 / np.sqrt(dim)) * cents + unit(randn(rng, NL, dim)), randn(rng, 4, dim)]))
    frozen(cents, of, rows, tail, queries)
    return cents, of, rows, tail, queries


def check_grid_fixture(dim):
    """on the CPU: the layout holds in every stored form, and every query's probes are safe for every nprobe used"""
    cents, of, rows, tail, queries = grid_case(dim)
    for dtype in DTYPES:
        best = (restate_rows(rows, dtype).astype(np.float64) @ cents.astype(np.float64).T).argmax(axis=1)
        assert np.array_equal(best, of), (dim, dtype)
    assert np.bincount(of, minlength=NL).tolist() == LENGTHS
    for nprobe in NPROBES:
        ref.probed_lists(queries, cents, nprobe)
    # query l probes list l first: at nprobe = 1 every list, the one-row list too, is scanned alone
    assert np.array_equal(ref.probed_lists(queries[:NL], cents, 1)[:, 0], np.arange(NL)), dim
    lists = np.concatenate([of, np.full(len(tail), -1)])
    per = ref.permitted_rows(lists, np.ones(len(lists), bool), ref.probed_lists(queries, cents, 1))
    assert per.sum(axis=1).min() == len(tail) and per.sum(axis=1).max() > 600      # k = 127 .. 256 exceed the permitted rows


@gpu
@pytest.mark.parametrize("dim", GRID_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_probed_search_grid(model, dtype, dim):
    check_grid_fixture(dim)
    cents, of, rows, tail, queries = grid_case(dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    ix.add(tail)
    both = np.concatenate([rows, tail])
    lists = ix.partition_lists()
    assert np.array_equal(lists[:len(rows)], of) and (lists[len(rows):] == -1).all()
    assert np.bincount(lists[lists >= 0], minlength=NL).tolist() == LENGTHS
    ref.check_lists(lists[:len(rows)], restate_rows(rows, dtype), cents, (dtype, dim))
    scores = ref.scores_of(queries, both, dtype)
    live = np.ones(len(both), bool)
    for nprobe in NPROBES:
        per = ref.permitted_rows(lists, live, ref.probed_lists(queries, cents, nprobe))
        for k in KS:
            got = ix.search_probed(queries, k, nprobe)
            ref.check_against_reference(got, dtype, queries, both, per, k, scores, (dtype, dim, nprobe, k))
            assert_same(got, ref.cross_check_by_filter(ix, queries, per, k), ("filter", dtype, dim, nprobe, k))
    assert_same(ix.search_probed(queries, 256, NL), ix.search(queries, 256), "every list probed is the search")
    ix.close()


@functools.lru_cache(maxsize=None)
def many_lists_case():
    """dim 130, 1500 rows over 300 lists, 9 Gaussian queries"""
    rng = np.random.default_rng(300)
    cents = ref.sign_centroids(rng, 300, 130)
    of = rng.integers(0, 300, 1500)
    rows = ref.rows_around(rng, cents, of)
    queries = unit(randn(rng, 9, 130))
    frozen(cents, of, rows, queries)
    return cents, of, rows, queries


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_probed_search_of_256_of_300_lists(model, dtype):
    cents, of, rows, queries = many_lists_case()
    ix = model.index(dim=130, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    lists = ix.partition_lists()
    assert np.array_equal(lists, of)
    scores = ref.scores_of(queries, rows, dtype)
    for nprobe, k in ((256, 256), (255, 129), (3, 256)):
        per = ref.permitted_rows(lists, np.ones(len(rows), bool), ref.probed_lists(queries, cents, nprobe))
        got = ix.search_probed(queries, k, nprobe)
        ref.check_against_reference(got, dtype, queries, rows, per, k, scores, (dtype, nprobe, k))
        assert_same(got, ref.cross_check_by_filter(ix, queries, per, k), ("filter", dtype, nprobe, k))
    ix.close()


# ---- 3. tail chunks

TAILS = [0, 1, 1023, 1024, 1025, 2500]
N_PART = 1500
# tail position -> the query whose own direction, three times as long, is the row there: the first and the last row of a chunk
# of 1024 and the last of the second chunk; 1026, 1027 and 2050 take those positions once three rows before them are compacted away
SPECIAL = {1023: 0, 1024: 1, 2047: 2, 1026: 3, 1027: 4, 2050: 5}
GONE_TAIL = [5, 500, 1000, 2200, 2499]                               # removed tail positions: three before 1023, none in 1023 .. 2050


@functools.lru_cache(maxsize=None)
def tail_case():
    rng = np.random.default_rng(130)
    cents = ref.sign_centroids(rng, 12, 130)
    of = rng.integers(0, 12, N_PART)
    rows = ref.rows_around(rng, cents, of)
    queries = unit(randn(rng, 8, 130))
    tail = unit(randn(rng, 2500, 130))
    for p, j in SPECIAL.items():
        tail[p] = 3 * queries[j]
    gone = np.concatenate([rng.choice(N_PART, 60, replace=False), N_PART + np.array(GONE_TAIL)]).astype(np.int32)
    frozen(cents, of, rows, queries, tail, gone)
    return cents, of, rows, queries, tail, gone


def check_tail(ix, dtype, queries, rows, lists, live, cents, n_part, found, what):
    """probed searches with nprobe = 1 against the reference and the filtered search; found: tail position -> query whose
    best row it must be"""
    scores = ref.scores_of(queries, rows, dtype)
    per = ref.permitted_rows(lists, live, ref.probed_lists(queries, cents, 1))
    for k in (1, 10, 200):
        got = ix.search_probed(queries, k, 1)
        ref.check_against_reference(got, dtype, queries, rows, per, k, scores, (what, dtype, k))
        assert_same(got, ref.cross_check_by_filter(ix, queries, per, k), ("filter", what, dtype, k))
        for p, j in found.items():
            assert got[0][j, 0] == n_part + p, (what, dtype, k, p, got[0][j, :4])
    return got


@gpu
@pytest.mark.parametrize("T", TAILS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_chunks(model, dtype, T):
    cents, of, rows, queries, tail, _ = tail_case()
    ix = model.index(dim=130, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    if T:
        assert ix.add(tail[:T]) == N_PART
    both = np.concatenate([rows, tail[:T]])
    lists = ix.partition_lists()
    assert np.array_equal(lists[:N_PART], of) and (lists[N_PART:] == -1).all() and len(lists) == N_PART + T
    found = {p: j for p, j in SPECIAL.items() if p < T}
    got = check_tail(ix, dtype, queries, both, lists, np.ones(len(both), bool), cents, N_PART, found, ("tail", T))
    if T >= 1023:
        assert (got[0] >= N_PART).any(axis=1).all()                  # (k = 200: one list of a dozen holds fewer rows)
    ix.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_with_removed_rows_and_after_compaction(model, dtype):
    cents, of, rows, queries, tail, gone = tail_case()
    ix = model.index(dim=130, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    ix.add(tail)
    both = np.concatenate([rows, tail])
    lists = ix.partition_lists()
    assert ix.remove(gone) == len(gone)
    live = np.ones(len(both), bool)
    live[gone] = False
    assert np.array_equal(ix.partition_lists(), lists)
    check_tail(ix, dtype, queries, both, lists, live, cents, N_PART, SPECIAL, "removed")
    old = ix.compact()
    assert np.array_equal(old, np.nonzero(live)[0])
    lists2 = ix.partition_lists()
    assert np.array_equal(lists2, lists[old])
    n_part = int((lists2 >= 0).sum())
    assert n_part == N_PART - 60 and len(ix) == len(both) - len(gone)
    shifted = {p - 3: j for p, j in SPECIAL.items()}                 # three rows of the tail before them are gone
    assert {1023, 1024, 2047} <= set(shifted)
    check_tail(ix, dtype, queries, both[old], lists2, np.ones(len(old), bool), cents, n_part, shifted, "compacted")
    ix.close()


# ---- 4. more than one chunk of queries

NQ_CHUNKS = 4097
CHECKED = [0, 4095, 4096]


@functools.lru_cache(maxsize=None)
def chunk_case():
    """dim 72, 1500 rows over 12 lists and a tail of 100, 4097 queries, 33 candidates each"""
    rng = np.random.default_rng(4097)
    cents = ref.sign_centroids(rng, 12, 72)
    of = rng.integers(0, 12, 1500)
    rows = ref.rows_around(rng, cents, of)
    tail = unit(randn(rng, 100, 72))
    queries = unit(randn(rng, NQ_CHUNKS, 72))
    cand = ref.candidates(rng, NQ_CHUNKS, 33, 1600, True)
    frozen(cents, of, rows, tail, queries, cand)
    return cents, of, rows, tail, queries, cand


@gpu
@pytest.mark.parametrize("dtype", ["f16", "b1"])
def test_device_entries_with_4097_queries(model, dtype):
    cents, of, rows, tail, queries, cand = chunk_case()
    Q, k, nprobe, n_cand = NQ_CHUNKS, 10, 2, cand.shape[1]
    ix = model.index(dim=72, dtype=dtype)
    ix.add(rows)
    ix.partition(cents)
    ix.add(tail)
    both = np.concatenate([rows, tail])
    lists = ix.partition_lists()
    assert np.array_equal(lists[:1500], of)
    live = np.ones(len(both), bool)
    hip = ref.Hip()
    s = hip.stream()
    d_q, d_c, d_i, d_s = hip.upload(queries), hip.upload(cand), hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
    # the probed search
    host = ix.search_probed(queries, k, nprobe)
    ix.search_probed_device(Q, d_q, nprobe, k, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), host, "probed: device entry")
    assert_same(ix.search_probed(queries[4096:], k, nprobe), (host[0][4096:], host[1][4096:]), "probed: query 4096 alone")
    qs = queries[CHECKED]
    per = ref.permitted_rows(lists, live, ref.probed_lists(qs, cents, nprobe))
    ref.check_against_reference((host[0][CHECKED], host[1][CHECKED]), dtype, qs, both, per, k, None, ("probed", dtype))
    # the rescore
    host = ix.rescore(queries, cand, k)
    ix.rescore_device(Q, d_q, n_cand, d_c, k, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), host, "rescore: device entry")
    per = np.zeros((len(CHECKED), len(both)), bool)
    for i, q in enumerate(CHECKED):
        per[i, cand[q][cand[q] >= 0]] = True
    ref.check_against_reference((host[0][CHECKED], host[1][CHECKED]), dtype, qs, both, per, k, None, ("rescore", dtype))
    hip.free(d_q, d_c, d_i, d_s)
    ix.close()


# ---- 5. the rescore grid

RESCORE_DIMS = [7, 384, 768, 2048]
RESCORE_SHAPES = [(1, (1, 3)), (33, (10, 40)), (1024, (128, 256))]  # n_cand, ks


@functools.lru_cache(maxsize=None)
def rescore_case(dim):
    """1500 unit rows with ten duplicates, 100 of them to be removed, five queries"""
    rng = np.random.default_rng(5000 + dim)
    rows = unit(randn(rng, 1500, dim))
    rows[100:110] = rows[100]
    queries = unit(randn(rng, 5, dim))
    gone = rng.choice(1500, 100, replace=False).astype(np.int32)
    frozen(rows, queries, gone)
    return rows, queries, gone


@gpu
@pytest.mark.parametrize("dim", RESCORE_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rescore_grid(model, dtype, dim):
    rows, queries, gone = rescore_case(dim)
    N, Q = len(rows), len(queries)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    assert ix.remove(gone) == len(gone)
    live = np.ones(N, bool)
    live[gone] = False
    scores = ref.scores_of(queries, rows, dtype)
    rng = np.random.default_rng(dim)
    hip = ref.Hip()
    s = hip.stream()
    d_q = hip.upload(queries)
    for n_cand, ks in RESCORE_SHAPES:
        cand = ref.candidates(rng, Q, n_cand, N, True)
        per = np.zeros((Q, N), bool)
        for i in range(Q):
            per[i, cand[i][cand[i] >= 0]] = True
        per &= live
        # the device call treats ids outside [0, size) as -1
        wild = cand.copy()
        wild[cand == -1] = rng.choice([-5, N, N + 77, 2 ** 31 - 1, -2 ** 31], int((cand == -1).sum()))
        d_c = hip.upload(wild)
        for k in ks:
            got = ix.rescore(queries, cand, k)
            ref.check_against_reference(got, dtype, queries, rows, per, k, scores, (dtype, dim, n_cand, k))
            assert_same(got, ref.cross_check_by_filter(ix, queries, per, k), ("filter", dtype, dim, n_cand, k))
            d_i, d_s = hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
            ix.rescore_device(Q, d_q, n_cand, d_c, k, d_i, d_s, s)
            assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), got, ("device", dtype, dim, n_cand, k))
            hip.free(d_i, d_s)
        hip.free(d_c)
    hip.free(d_q)
    ix.close()


# ---- without a GPU: the fixtures' assertions, and the references against each other

@pytest.mark.parametrize("dim", GRID_DIMS)
def test_grid_fixture_margins_and_list_lengths(dim):
    check_grid_fixture(dim)


def test_f32_chain_meets_the_tolerance_on_the_grid_fixture():
    """a correctly rounded f32 fma chain in the kernel's order, on every (query, row) of the largest dim, is within the
    tolerance the GPU result is held to, with room: the fixture asks nothing of the kernel that its arithmetic cannot give"""
    cents, of, rows, tail, queries = grid_case(2048)
    both = np.concatenate([rows, tail])
    fs = ref.FloatScores(queries, both, "f32")
    ratio = np.abs(ref.f32_chain_scores(queries, both).astype(np.float64) - fs.exact) / fs.tol
    print(f"f32 chain, dim 2048: worst err / tol {ratio.max():.3f}")
    assert ratio.max() < 0.5


def test_other_fixtures_margins():
    cents, of, rows, queries = many_lists_case()
    for dtype in DTYPES:
        assert np.array_equal((restate_rows(rows, dtype).astype(np.float64) @ cents.astype(np.float64).T).argmax(axis=1), of)
    for nprobe in (256, 255, 3):
        ref.probed_lists(queries, cents, nprobe)
    cents, of, rows, queries, tail, gone = tail_case()
    ref.probed_lists(queries, cents, 1)
    both = np.concatenate([rows, tail])
    assert not np.isin(N_PART + np.array(list(SPECIAL)), gone).any()
    for dtype in DTYPES:
        assert np.array_equal((restate_rows(rows, dtype).astype(np.float64) @ cents.astype(np.float64).T).argmax(axis=1), of)
        # the distinctive rows are the best rows of their queries by the reference itself, far beyond any tolerance
        s = ref.scores_of(queries, both, dtype)
        s = s if isinstance(s, np.ndarray) else s.exact
        for p, j in SPECIAL.items():
            rest = np.delete(s[j], N_PART + p)
            assert s[j, N_PART + p] > 1.5 * rest.max() > 0, (dtype, p)
    cents, of, rows, tail, queries, cand = chunk_case()
    ref.probed_lists(queries[CHECKED], cents, 2)


@pytest.mark.parametrize("dim", [1, 7, 130, 2048])
def test_integer_restatements_agree_with_float64(dim):
    """((float)dot * qs) * rs is two roundings of the exact product, (float)dot * qs one: the restated i8 and b1 scores lie
    within (1 + u)^2 - 1 and u of float64 arithmetic on the same codes and scales"""
    rng = np.random.default_rng(dim)
    rows, queries = randn(rng, 200, dim), randn(rng, 7, dim)
    qc, qs = ref.quantize(queries)
    rc, rs = ref.quantize(rows)
    exact = (qc.astype(np.float64) @ rc.astype(np.float64).T) * qs.astype(np.float64)[:, None] * rs.astype(np.float64)[None, :]
    assert (np.abs(ref.exact_scores(queries, rows, "i8") - exact) <= (2 * ref.U + ref.U ** 2) * np.abs(exact)).all()
    exact = (qc.astype(np.float64) @ np.where(rows > 0, 1.0, -1.0).T) * qs.astype(np.float64)[:, None]
    assert (np.abs(ref.exact_scores(queries, rows, "b1") - exact) <= ref.U * np.abs(exact)).all()
    # and the i8 scores are the float64 scores of the restated rows and queries up to those roundings and the ones of
    # code * scale: 4 u in all to first order
    r64, q64 = restate_rows(rows, "i8").astype(np.float64), restate_rows(queries, "i8").astype(np.float64)
    assert (np.abs(ref.exact_scores(queries, rows, "i8") - q64 @ r64.T) <= 5 * ref.U * (np.abs(q64) @ np.abs(r64).T)).all()


def test_float_rule_accepts_the_exact_answer_and_rejects_a_wrong_one():
    rng = np.random.default_rng(9)
    rows, queries = unit(randn(rng, 300, 130)), unit(randn(rng, 4, 130))
    for dtype in ("f32", "f16"):
        fs = ref.FloatScores(queries, rows, dtype)
        per = rng.random((4, 300)) < 0.5
        per[3] = False
        per[3, :5] = True
        k = 10
        ids, sc = ref.ref_topk(np.where(per, fs.exact, np.nan), k)
        sc = sc.astype(np.float32)
        ref.check_float((ids, sc), fs, per, k)
        assert (ids[3, 5:] == -1).all()
        # a missing best row, a row that is not permitted, a score off by ten tolerances, an order by id where scores differ
        wrong = []
        a = ids.copy(), sc.copy()
        a[0][0, :-1], a[1][0, :-1] = ids[0, 1:], sc[0, 1:]
        a[0][0, -1], a[1][0, -1] = ids[0, 0], -1.0
        wrong.append(a)
        a = ids.copy(), sc.copy()
        a[0][1, 4] = np.nonzero(~per[1])[0][0]
        wrong.append(a)
        a = ids.copy(), sc.copy()
        a[1][2, 0] += np.float32(10 * fs.tol[2, ids[2, 0]])
        wrong.append(a)
        a = ids.copy(), sc.copy()
        a[0][3, 5] = 7
        wrong.append(a)
        for a in wrong:
            with pytest.raises(AssertionError):
                ref.check_float(a, fs, per, k)


def test_list_rule_accepts_the_argmax_and_the_smallest_tied_list_only():
    rng = np.random.default_rng(3)
    rows, cents = randn(rng, 50, 7), randn(rng, 9, 7)
    cents[6] = cents[2]
    rows[4] = 0.0
    lists = (rows.astype(np.float64) @ cents.astype(np.float64).T).argmax(axis=1)
    assert lists[4] == 0 and not (lists == 6).any() and (lists == 2).any()
    ref.check_lists(lists, rows, cents)
    for row, to in ((int(np.nonzero(lists == 2)[0][0]), 6), (4, 1), (0, (lists[0] + 1) % 9)):
        bad = lists.copy()
        bad[row] = to
        with pytest.raises(AssertionError):
            ref.check_lists(bad, rows, cents)
    # the probe margin refuses a ranking that f32 could change
    near = np.stack([cents[0], cents[0] * np.float32(1 + 2e-7), cents[1]])
    with pytest.raises(AssertionError):
        ref.probed_lists(np.abs(rows[:3]) * np.sign(cents[0]), near, 1)
