"""The selecting kernels on ordered and exact-fit score sequences: index_topk_kernel, index_probe_kernel and topk_merge_kernel
(search.hip) and sparse_index_scan_kernel (sparse_index.hip), plain and masked, against the order rule over scores that are exact in
every accumulation order (tests/topk_order_reference.py).  Every comparison is bit for bit, ids and scores.

Random scores fill a candidate queue once; these fill it at every step, fill it exactly (count == room, so the step is not sorted and
the next one writes up to the list's last slot), keep one query of a tile busy beside idle ones, and tie over the whole index.
test_topk_order_host.py proves on the CPU, with a model of the queue, that each fixture used here reaches the state it is built for."""
import numpy as np
import pytest

import index_reference as ixr
import sparse_index_reference as sref
import test_gpu_sparse_index as tsi
import topk_order_reference as tor

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    """any model: an index only needs the context's device.  It profiles, so that the last test can show which kernels this file ran."""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    yield m
    m.close()


def per_kind(fx, k, ok=None):
    """kind -> the reference's (ids [1, k], scores [1, k]) over the rows a search may return (ok: another allow-list), once per fixture"""
    return {kk: tor.reference_topk(fx.scores[kk][None], fx.permitted() if ok is None else ok, k) for kk in fx.kinds}


def of_layout(want, lay):
    return np.concatenate([want[kk][0] for kk in lay]), np.concatenate([want[kk][1] for kk in lay])


# ------------------------------------------------------------------------------------------------
# index_topk_kernel
# ------------------------------------------------------------------------------------------------
def dense_index(model, fx, mode):
    ix = model.index(dim=fx.rows.shape[1], dtype=fx.dtype)
    ix.add(fx.rows)
    if mode == "removed":
        gone = np.nonzero(~fx.ok)[0]
        assert ix.remove(gone) == len(gone) and ix.n_live == fx.n - len(gone)
    return ix


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.DENSE_KS)
@pytest.mark.parametrize("dtype", tor.DENSE_DTYPES)
def test_dense_search_on_ordered_and_exact_fit_rows(model, dtype, k, mode):
    for fx in tor.dense_fixtures(dtype, k, mode):
        ix = dense_index(model, fx, mode)
        allow = fx.ok if mode == "allow" else None
        want = per_kind(fx, k)
        want1 = per_kind(fx, k, fx.ok1) if mode == "allow" else None
        for nq in tor.DENSE_NQS:
            for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tor.QT).items():
                q = np.stack([fx.queries[kk] for kk in lay])
                ixr.assert_same(ix.search(q, k, allow=allow), of_layout(want, lay), (fx.name, nq, name))
                if mode == "allow":                                  # the near miss of the same index: one row more than fits
                    ixr.assert_same(ix.search(q, k, allow=fx.ok1), of_layout(want1, lay), (fx.name, "near miss", nq, name))
        if mode == "removed":
            # removed rows and an allow-list of the same rows: one mask
            lay = tor.layouts(fx.kinds, fx.busy, fx.idle, 33, tor.QT)["mixed"]
            q = np.stack([fx.queries[kk] for kk in lay])
            ixr.assert_same(ix.search(q, k, allow=fx.ok), of_layout(want, lay), (fx.name, "removed and disallowed"))
        ix.close()


# ------------------------------------------------------------------------------------------------
# many slices: topk_merge_kernel's outer rounds and its refill
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(model):
    """f32 rows only (the merge does not know the form): a dense and a sparse index of at least 17 slices at k = 256"""
    n = tor.MANY_DENSE_ROWS
    rows = np.zeros((n, tor.FLOAT_DIM), np.float32)
    rows[:, 0] = 1 + np.arange(n)
    dense = model.index(dim=tor.FLOAT_DIM, dtype="f32")
    dense.add(rows)
    sparse = model.sparse_index(1, "f32", n_vocab=tor.SPARSE_V)
    sparse.add(*tor.many_sparse_rows())
    yield dense, sparse
    dense.close()
    sparse.close()


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_many_slices_and_a_second_merge_round(model, many, k):
    dense, sparse = many
    for ix, n, is_sparse in ((dense, tor.MANY_DENSE_ROWS, False), (sparse, tor.MANY_SPARSE_ROWS, True)):
        sc = tor.many_scores(n)
        want = {kk: tor.reference_topk(sc[kk][None], True, k) for kk in sc}
        assert want["asc"][0][0, 0] == n - 1 and want["desc"][0][0].tolist() == list(range(k)) == want["const"][0][0].tolist()
        for nq in tor.MANY_NQS:
            if is_sparse:
                slices = pybert.test_sparse_scan_geometry(0, tor.SPARSE_V, n, nq, k)["n_slices"]
            else:
                slices = pybert.test_index_plan(n, nq, k)["slices"]
            assert slices >= 17 and (k != 256 or slices * k > tor.MERGE_OUTER)
            lay = tor.many_layout(nq)
            if is_sparse:
                got = ix.search(*tor.sparse_query(lay), k)
            else:
                got = ix.search(np.stack([tor.dense_query("f32", 0, {"asc": 1, "desc": -1, "const": 0}[kk]) for kk in lay]), k)
            ixr.assert_same(got, of_layout(want, lay), ("sparse" if is_sparse else "dense", k, nq))


@pytest.mark.parametrize("k", tor.MERGE_KS)
def test_rescored_candidates_and_the_merge_s_exact_fit(model, k):
    """a rescore hands the merge 1024 candidates in the caller's order: its own staircase (a round that fills the queue exactly, then a
    whole round, up to slot 511) and the near miss, through the dense and the sparse rescore"""
    sc = tor.merge_scores(k)
    want = of_layout({kk: tor.reference_topk(sc[kk][None], True, k) for kk in sc}, tor.MERGE_KINDS)
    cand = np.tile(np.arange(tor.MERGE_CAND, dtype=np.int32), (len(tor.MERGE_KINDS), 1))
    rows = np.zeros((tor.MERGE_CAND, tor.FLOAT_DIM), np.float32)
    rows[:, 0], rows[:, 1] = sc["stair"], sc["over"]
    q = np.zeros((len(tor.MERGE_KINDS), tor.FLOAT_DIM), np.float32)
    for i, kk in enumerate(tor.MERGE_KINDS):
        col, sign = tor.MERGE_COLUMN[kk]
        if col >= 0:
            q[i, col] = sign
    for dtype in ("f32", "f16"):
        ix = model.index(dim=tor.FLOAT_DIM, dtype=dtype)
        ix.add(rows)
        ixr.assert_same(ix.rescore(q, cand, k), want, ("dense rescore", dtype, k))
        ix.close()
    ix = model.sparse_index(2, "f32", n_vocab=tor.SPARSE_V)
    ix.add(np.tile(np.array([0, 1], np.int32), (tor.MERGE_CAND, 1)), rows[:, :2])
    q_ids = np.array([[tor.MERGE_COLUMN[kk][0]] for kk in tor.MERGE_KINDS], np.int32)
    q_w = np.array([[tor.MERGE_COLUMN[kk][1]] for kk in tor.MERGE_KINDS], np.float32)
    ixr.assert_same(ix.rescore(q_ids, q_w, cand, k), want, ("sparse rescore", k))
    ix.close()


# ------------------------------------------------------------------------------------------------
# index_probe_kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tor.PROBE_FORMS)
@pytest.mark.parametrize("k", tor.PROBE_KS)
@pytest.mark.parametrize("dtype", tor.DENSE_DTYPES)
def test_probed_search_on_ordered_and_exact_fit_lists(model, dtype, k, form):
    fx = tor.probe_fixture(dtype, k, form)
    masked = form == "allow"
    ix, fine = (model.index(dim=fx.rows.shape[1], dtype=dtype) for _ in range(2))
    ix.add(fx.rows[:fx.n_part])
    ix.partition(fx.centroids)
    ix.add(fx.rows[fx.n_part:])
    fine.add(fx.rows)
    assert np.array_equal(ix.partition_lists(), fx.lists)            # membership is by construction
    lay = tor.probe_layout()
    q = np.stack([fx.queries[kk] for kk in lay])
    want = of_layout(per_kind(fx, k), lay)
    allow = fx.ok if masked else None
    got = ix.search_probed(q, k, tor.PROBE_LISTS, allow=allow)
    ixr.assert_same(got, want, fx.name)
    if masked:
        ixr.assert_same(ix.search_probed(q, k, tor.PROBE_LISTS, allow=fx.ok1), of_layout(per_kind(fx, k, fx.ok1), lay), (fx.name, "near miss"))
    # the documented equivalents: one search with the same rows allowed; a two-stage search whose fine index scores alike
    ixr.assert_same(got, ix.search(q, k, allow=fx.permitted()), (fx.name, "search(allow)"))
    ixr.assert_same(ix.search_rescored_probed(fine, q, k, max(k, 200), tor.PROBE_LISTS, allow=allow), want, (fx.name, "rescored"))
    ixr.assert_same(ix.search_rescored(fine, q, k, 256), tor.reference_topk(fx.S(lay), True, k), (fx.name, "rescored, not probed"))
    ix.close()
    fine.close()


# ------------------------------------------------------------------------------------------------
# sparse_index_scan_kernel
# ------------------------------------------------------------------------------------------------
SPARSE_NQS = (1, 2, 3, 5)


def sparse_index(model, fx, mode):
    ix = model.sparse_index(fx.width, fx.dtype, n_vocab=tor.SPARSE_V)
    ix.add(fx.term_ids, fx.term_w)
    if mode == "removed":
        gone = np.nonzero(~fx.ok)[0]
        assert ix.remove(gone) == len(gone)
    return ix


def sparse_layouts(ix, fx, k, nqs, allow, qb=None):
    """every layout of every nq against the reference; the tile is the one the plan gives under the tuning key's value qb"""
    want = per_kind(fx, k, allow)
    for nq in nqs:
        g = pybert.test_sparse_scan_geometry(tor.SPARSE_DTYPES.index(fx.dtype), tor.SPARSE_V, fx.n, nq, k, qb=qb)
        assert g["qb"] == min(2 if qb is None else qb, nq), g
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, g["qb"]).items():
            ixr.assert_same(ix.search(*tor.sparse_query(lay), k, allow=allow), of_layout(want, lay), (fx.name, qb, nq, name))


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.SPARSE_KS)
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_sparse_search_on_ordered_and_exact_fit_rows(model, dtype, k, mode):
    fx = tor.sparse_fixture(dtype, k, mode)
    ix = sparse_index(model, fx, mode)
    sparse_layouts(ix, fx, k, SPARSE_NQS, fx.ok if mode == "allow" else None)
    if mode == "allow":
        sparse_layouts(ix, fx, k, SPARSE_NQS, fx.ok1)             # the near miss: one row more than fits
    ix.close()


# ------------------------------------------------------------------------------------------------
# the sparse scan's tile sizes (the tuning key "sparse_index_qb")
# ------------------------------------------------------------------------------------------------
TILES = (1, 2, 3, 4, 5, 8)
TILE_CASES = ("V 1000", "V 30522, two slices", "V 262144, the largest query image")


@pytest.fixture(scope="module")
def tile_cases(model):
    """the random cases of test_gpu_sparse_index.py on this file's model, with their reference results by k, and the ordered tile"""
    out = {}
    for case in tsi.SEARCH_CASES:
        if case[0] in TILE_CASES:
            ix, q_ids, q_w, sc = tsi.build_search_case(model, case)
            want = {}
            for k in (1, 10, 256):
                res = [sref.topk(s, k) for s in sc]
                want[k] = np.stack([x[0] for x in res]), np.stack([x[1] for x in res])
            out[case[0]] = (case, ix, q_ids, q_w, want)
    assert len(out) == len(TILE_CASES)
    ordered = {}
    for mode in ("plain", "allow"):
        fx = tor.sparse_fixture("f32", 128, mode)
        ordered[mode] = (fx, sparse_index(model, fx, mode))
    yield out, ordered
    for _, ix, _, _, _ in out.values():
        ix.close()
    for _, ix in ordered.values():
        ix.close()


def random_case_under_tile(entry, qb, tile_wanted=None):
    case, ix, q_ids, q_w, want = entry
    name, V, dtype, rows = case[0], case[1], case[2], case[5]
    for k in (1, 10, 256):
        for nq in sorted({1, 2, max(qb, 1) - 1, max(qb, 1), max(qb, 1) + 1, tsi.NQ} - {0}):
            g = pybert.test_sparse_scan_geometry(tsi.DTYPES.index(dtype), V, rows, nq, k, qb=qb)
            if tile_wanted is not None:
                assert g["qb"] == min(tile_wanted, nq), (name, qb, g)
            got = ix.search(q_ids[:nq], q_w[:nq], k)
            ixr.assert_same(got, (want[k][0][:nq], want[k][1][:nq]), (name, qb, k, nq))
    return g


@pytest.mark.parametrize("n", TILES)
def test_sparse_tile_sizes(model, tile_cases, n):
    cases, ordered = tile_cases
    try:
        model.set_option("sparse_index_qb", str(n))
        for name in TILE_CASES[:2]:
            random_case_under_tile(cases[name], n, tile_wanted=n)
        for mode, (fx, ix) in ordered.items():
            sparse_layouts(ix, fx, 128, sorted({n - 1, n, n + 1, 70} - {0}), fx.ok if mode == "allow" else None, qb=n)
    finally:
        model.set_option("sparse_index_qb", "0")


def test_sparse_tile_the_lds_clamp_and_values_out_of_range(model, tile_cases):
    cases, _ = tile_cases
    try:
        # the largest query image: the LDS takes fewer than the 8 asked for (3 with lists of 512 entries, 2 with lists of 1024)
        model.set_option("sparse_index_qb", "8")
        for k, tile in ((10, 3), (256, 2)):
            g = pybert.test_sparse_scan_geometry(0, 262144, 130, tsi.NQ, k, qb=8)
            assert 1 <= g["qb"] < 8 and g["qb"] == tile, g
        random_case_under_tile(cases[TILE_CASES[2]], 8)
        # values outside 1 .. 8 are the table's tile
        table = pybert.test_sparse_scan_geometry(1, 30522, 5000, tsi.NQ, 10)
        for bad in (0, 9, -1):
            model.set_option("sparse_index_qb", str(bad))
            assert pybert.test_sparse_scan_geometry(1, 30522, 5000, tsi.NQ, 10, qb=bad) == table
            random_case_under_tile(cases[TILE_CASES[1]], bad, tile_wanted=table["qb"])
    finally:
        model.set_option("sparse_index_qb", "0")


# ------------------------------------------------------------------------------------------------
# which kernels this file ran
# ------------------------------------------------------------------------------------------------
def test_every_selecting_kernel_ran_under_this_file(model):
    """a small search per kernel and instantiation of its own (so that the test stands alone), then the profiler's launch counts, which
    after a run of the whole file hold every test above"""
    for dtype in tor.DENSE_DTYPES:
        fx = tor.dense_fixtures(dtype, 128, "allow")[0]
        ix = dense_index(model, fx, "allow")
        q = np.stack([fx.queries[kk] for kk in fx.kinds])
        ixr.assert_same(ix.search(q, 128), of_layout({kk: tor.reference_topk(fx.scores[kk][None], True, 128) for kk in fx.kinds}, fx.kinds), dtype)
        ixr.assert_same(ix.search(q, 128, allow=fx.ok), of_layout(per_kind(fx, 128), fx.kinds), dtype)
        ix.close()
        fx = tor.probe_fixture(dtype, 128, "allow")
        ix = model.index(dim=fx.rows.shape[1], dtype=dtype)
        ix.add(fx.rows[:fx.n_part])
        ix.partition(fx.centroids)
        ix.add(fx.rows[fx.n_part:])
        q = np.stack([fx.queries[kk] for kk in fx.kinds])
        ixr.assert_same(ix.search_probed(q, 128, tor.PROBE_LISTS), tor.reference_topk(fx.S(fx.kinds), True, 128), dtype)
        ixr.assert_same(ix.search_probed(q, 128, tor.PROBE_LISTS, allow=fx.ok), of_layout(per_kind(fx, 128), fx.kinds), dtype)
        ix.close()
    for dtype in tor.SPARSE_DTYPES:
        fx = tor.sparse_fixture(dtype, 128, "allow")
        ix = sparse_index(model, fx, "allow")
        ixr.assert_same(ix.search(*tor.sparse_query(fx.kinds), 128),
                        of_layout({kk: tor.reference_topk(fx.scores[kk][None], True, 128) for kk in fx.kinds}, fx.kinds), dtype)
        ixr.assert_same(ix.search(*tor.sparse_query(fx.kinds), 128, allow=fx.ok), of_layout(per_kind(fx, 128), fx.kinds), dtype)
        ix.close()
    rep = model.profile_report()
    names = [f"index_topk_{d}{m}" for d in tor.DENSE_DTYPES for m in ("", "_masked")]
    names += [f"index_probe_{d}{m}" for d in tor.DENSE_DTYPES for m in ("", "_masked")]
    names += [f"sparse_index_scan_{d}{m}" for d in tor.SPARSE_DTYPES for m in ("", "_masked")] + ["topk_merge"]
    for name in names:
        print(f"{name}: {rep.get(name, {}).get('launches', 0)} launches")
    for name in names:
        assert rep.get(name, {}).get("launches", 0) >= 1, (name, sorted(rep))
