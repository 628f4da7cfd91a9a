"""sparse_postings_scan_kernel (sparse_postings.hip) on ordered and exact-fit scores and over walked segments, plain and masked, f32
and f16 rows.  Every comparison is bit for bit, ids and scores, against the order rule (tor.reference_topk, or the sparse reference
for the random cases); where said, also against the row-major search of the same object.

The inverted scan keeps its own copy of the selection loop — push, count, room = L - k - 256, sort and refresh — inside a loop over the
segments of a slice, and its other tests give every workgroup one segment of random scores.  Here a workgroup walks up to 16 segments
with one query of its tile busy and the others idle, fills its queue exactly and one row beyond, takes more than 64 KiB of LDS for
segments of 8192 and 16384 rows, and hands the merge 17 lists a query.  tests/topk_order_reference.py INVERTED_CELLS lists the launch
geometries; test_sparse_inverted_order_host.py proves on the CPU, from the plan's hook and a model of the queue, that each reaches what
it is listed for."""
import numpy as np
import pytest

import index_reference as ixr
import sparse_index_reference as sref
import sparse_inverted_cases as cases
import topk_order_reference as tor

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

HOOK = pybert.test_sparse_postings_geometry


@pytest.fixture(scope="module")
def model(make_model):
    """any model: an index only needs the context's device.  It profiles, so that the last test can show which kernels this file ran."""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    yield m
    m.set_option("sparse_index_segment_rows", "0")
    m.set_option("sparse_index_qb", "0")
    m.close()


def invert(model, ix, seg):
    """the postings of ix in segments of seg rows; the key goes back to 0 (invert has read it)"""
    try:
        model.set_option("sparse_index_segment_rows", str(seg))
        assert ix.invert() == len(ix) == ix.inverted_rows
    finally:
        model.set_option("sparse_index_segment_rows", "0")


def sparse_index(model, fx, mode):
    ix = model.sparse_index(fx.width, fx.dtype, n_vocab=tor.SPARSE_V)
    ix.add(fx.term_ids, fx.term_w)
    if mode == "removed":
        gone = np.nonzero(~fx.ok)[0]
        assert ix.remove(gone) == len(gone)
    return ix


def per_kind(fx, k, ok=None):
    """kind -> the reference's (ids [1, k], scores [1, k]) over the rows a search may return (ok: another allow-list), once per fixture"""
    return {kk: tor.reference_topk(fx.scores[kk][None], fx.permitted() if ok is None else ok, k) for kk in fx.kinds}


def run_cell(ix, fx, cell, allow, want):
    """every layout of a cell against the per-kind reference; the tile is the plan's under the cell's key"""
    plan = tor.postings_plan(HOOK, tor.SPARSE_DTYPES.index(fx.dtype), fx.n, cell.nq, cell.k, cell.seg, cell.qb)
    tor.check_inverted_geometry(cell, fx.n, plan)
    for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, cell.nq, plan[0][2]["qb"]).items():
        got = ix.search_inverted(*tor.sparse_query(lay), cell.k, allow=allow)
        ixr.assert_same(got, tor.of_layout(want, lay), (fx.name, cell, name))


def run_cells(model, ix, fx, cells, mode):
    """the cells of one fixture, segment size by segment size: the exact fit, and under an allow-list its near miss too"""
    k = cells[0].k
    want = per_kind(fx, k)
    want1 = per_kind(fx, k, fx.ok1) if mode == "allow" else None
    for seg in sorted({c.seg for c in cells}):
        invert(model, ix, seg)
        for cell in cells:
            if cell.seg == seg:
                run_cell(ix, fx, cell, fx.ok if mode == "allow" else None, want)
                if mode == "allow":
                    run_cell(ix, fx, cell, fx.ok1, want1)


# ------------------------------------------------------------------------------------------------
# 1. ordered and exact-fit rows in one segment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.SPARSE_KS)
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_ordered_and_exact_fit_rows_in_one_segment(model, dtype, k, mode):
    fx = tor.sparse_fixture(dtype, k, mode)
    ix = sparse_index(model, fx, mode)
    cells = tor.inverted_cells("one", k=k, mode=mode)
    assert len(cells) == len(tor.INVERTED_NQS)
    run_cells(model, ix, fx, cells, mode)
    if mode == "removed":
        # removed rows and an allow-list of the same rows: one mask
        lay = tor.layouts(fx.kinds, fx.busy, fx.idle, 5, 2)["mixed"]
        ixr.assert_same(ix.search_inverted(*tor.sparse_query(lay), k, allow=fx.ok), tor.of_layout(per_kind(fx, k), lay), (fx.name, "removed and disallowed"))
    ix.close()


# ------------------------------------------------------------------------------------------------
# 2. the same fixtures over walked segments: 2048 workgroups that each walk all 16 (or 4) segments, a second chunk, slices of 3 segments
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.INVERTED_WALKED_KS)
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_ordered_and_exact_fit_rows_over_walked_segments(model, dtype, k, mode):
    fx = tor.sparse_fixture(dtype, k, mode)
    ix = sparse_index(model, fx, mode)
    cells = tor.inverted_cells("walked", k=k, mode=mode)
    assert {(c.seg, c.nq) for c in cells} == set(tor.INVERTED_WALKED)
    run_cells(model, ix, fx, cells, mode)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 3. tiles (the tuning key "sparse_index_qb"; values beyond 4 aim for 4)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile_indexes(model):
    out = {}
    for mode in ("plain", "allow"):
        fx = tor.sparse_fixture("f32", tor.INVERTED_TILE_K, mode)
        out[mode] = (fx, sparse_index(model, fx, mode))
    yield out
    for _, ix in out.values():
        ix.close()


@pytest.mark.parametrize("n", tor.INVERTED_TILES)
def test_tile_sizes_on_ordered_rows(model, tile_indexes, n):
    try:
        model.set_option("sparse_index_qb", str(n))
        for mode, (fx, ix) in tile_indexes.items():
            run_cells(model, ix, fx, tor.inverted_cells("tiles", qb=n, mode=mode), mode)
    finally:
        model.set_option("sparse_index_qb", "0")


# ------------------------------------------------------------------------------------------------
# 4. more than 64 KiB of LDS, and row numbers beyond 2047 inside a segment
# ------------------------------------------------------------------------------------------------
BIG_RANDOM = dict(V=1000, width=4, nq=8, kq=32)


@pytest.fixture(scope="module")
def big(model):
    """per row type: the ordered index of 16384 + 300 rows, its twin with 200 rows around row 16383 removed, and a random index of as
    many rows of up to four terms with its reference scores"""
    n = tor.INVERTED_BIG_ROWS
    rng = np.random.default_rng(16384)
    r_ids, r_w = cases._terms(rng, n, BIG_RANDOM["width"], BIG_RANDOM["V"], BIG_RANDOM["width"], 2.0)
    q_ids, q_w = cases._terms(rng, BIG_RANDOM["nq"], BIG_RANDOM["kq"], BIG_RANDOM["V"], BIG_RANDOM["kq"], 2.0)
    out = {}
    for dtype in tor.SPARSE_DTYPES:
        ids, w, sc = tor.big_inverted_rows(dtype)
        whole, holed = (model.sparse_index(1, dtype, n_vocab=tor.SPARSE_V) for _ in range(2))
        for ix in (whole, holed):
            ix.add(ids, w)
        assert holed.remove(tor.INVERTED_BIG_GONE) == len(tor.INVERTED_BIG_GONE)
        rand = model.sparse_index(BIG_RANDOM["width"], dtype, n_vocab=BIG_RANDOM["V"])
        rand.add(r_ids, r_w)
        st = sref.stored_rows(r_ids, r_w, BIG_RANDOM["width"], dtype)
        rsc = sref.scores(st[0], st[1], q_ids, q_w, BIG_RANDOM["V"])
        out[dtype] = dict(sc=sc, whole=whole, holed=holed, rand=rand, rsc=rsc, q=(q_ids, q_w))
    yield out
    for d in out.values():
        for name in ("whole", "holed", "rand"):
            d[name].close()


@pytest.mark.parametrize("seg,k,tile", tor.INVERTED_BIG)
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_large_segments_more_than_64_kib_of_lds_and_high_row_numbers(model, big, dtype, seg, k, tile):
    n, b = tor.INVERTED_BIG_ROWS, big[dtype]
    sc = b["sc"]
    live = np.ones(n, bool)
    live[tor.INVERTED_BIG_GONE] = False
    first = np.arange(n) < 16384                                   # segment 0 of 16384 rows alone: the winners' row numbers reach 16383
    try:
        model.set_option("sparse_index_qb", str(tor.INVERTED_BIG_QB))
        for ix in (b["whole"], b["holed"], b["rand"]):
            invert(model, ix, seg)
        for nq in tor.INVERTED_BIG_NQS:
            (_, _, g), = tor.postings_plan(HOOK, tor.SPARSE_DTYPES.index(dtype), n, nq, k, seg, tor.INVERTED_BIG_QB)
            assert g["qb"] == min(tile, nq) and (nq < tor.INVERTED_BIG_QB or g["lds"] > tor.INVERTED_LDS_STATIC), g
            lay = tor.many_layout(nq)
            q = tor.sparse_query(lay)
            for ix, ok, allow, what in ((b["whole"], True, None, "all rows"), (b["holed"], live, None, "rows around the edge removed"),
                                        (b["whole"], first, first, "the first segment allowed"), (b["holed"], live & first, first, "removed and allowed")):
                want = {kk: tor.reference_topk(sc[kk][None], ok, k) for kk in sc}
                if dtype == "f32":
                    assert want["asc"][0][0, 0] == np.flatnonzero(np.broadcast_to(ok, n))[-1]          # the last row that qualifies wins
                assert want["desc"][0][0].tolist() == list(range(k)) == want["const"][0][0].tolist()
                ixr.assert_same(ix.search_inverted(*q, k, allow=allow), tor.of_layout(want, lay), (dtype, seg, k, nq, what))
        # random rows of up to four terms: winners anywhere in a segment
        (_, _, g), = tor.postings_plan(HOOK, tor.SPARSE_DTYPES.index(dtype), n, BIG_RANDOM["nq"], k, seg, tor.INVERTED_BIG_QB, BIG_RANDOM["V"])
        assert g["qb"] == tile and g["lds"] > tor.INVERTED_LDS_STATIC, g
        rnd = np.random.default_rng(seg + k).random(n) < 0.5
        for allow in (None, rnd):
            want = cases.want(b["rsc"], k, allow)
            got = b["rand"].search_inverted(*b["q"], k, allow=allow)
            ixr.assert_same(got, want, (dtype, seg, k, "random", allow is not None))
            ixr.assert_same(got, b["rand"].search(*b["q"], k, allow=allow), (dtype, seg, k, "random, the row-major search", allow is not None))
        assert (want[0] % seg > 2047).any() and (want[0] >= seg).any()
    finally:
        model.set_option("sparse_index_qb", "0")


# ------------------------------------------------------------------------------------------------
# 5. several segments per slice on random scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_random_scores_over_slices_of_three_and_two_segments(model, dtype):
    V, _, width = cases.CASES["a"][:3]
    rows, seg, T = cases.ROWS_SLICED, cases.SEG_TEST, cases.TILING
    ids, w, q_ids, q_w = cases.data("a", rows)
    sc = cases.scores("a", dtype, rows)
    Q_ids, Q_w = np.tile(q_ids, (T, 1)), np.tile(q_w, (T, 1))
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    invert(model, ix, seg)
    rng = np.random.default_rng(9)
    allow = rng.random(rows) < 0.3
    live = np.ones(rows, bool)

    def check(allowed, what):
        for k in (1, 10, 256):
            (_, _, g), = tor.postings_plan(HOOK, tor.SPARSE_DTYPES.index(dtype), rows, len(Q_ids), k, seg, 0, V)
            assert (g["n_qtiles"], g["n_segs"], g["slice_segs"], g["n_slices"]) == (525, 11, 3, 4), g
            one = cases.want(sc, k, live if allowed is None else live & allowed)
            want = np.tile(one[0], (T, 1)), np.tile(one[1], (T, 1))
            got = ix.search_inverted(Q_ids, Q_w, k, allow=allowed)
            ixr.assert_same(got, want, (dtype, what, k))
            ixr.assert_same(got, ix.search(Q_ids, Q_w, k, allow=allowed), (dtype, what, k, "the row-major search"))

    check(None, "plain")
    check(allow, "an allow-list")
    gone = rng.permutation(rows)[:700]
    assert ix.remove(gone) == 700 and ix.inverted_rows == rows
    live[gone] = False
    check(None, "removed rows")
    check(allow, "removed rows and an allow-list")
    ix.close()


# ------------------------------------------------------------------------------------------------
# 6. many slices: the merge's second outer round behind the inverted scan
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(model):
    ix = model.sparse_index(1, "f32", n_vocab=tor.SPARSE_V)
    ix.add(*tor.many_sparse_rows())
    invert(model, ix, cases.SEG_DEFAULT)
    yield ix
    ix.close()


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_many_slices_and_a_second_merge_round(model, many, k):
    n = tor.MANY_SPARSE_ROWS
    sc = tor.many_scores(n)
    want = {kk: tor.reference_topk(sc[kk][None], True, k) for kk in sc}
    assert want["asc"][0][0, 0] == n - 1 and want["desc"][0][0].tolist() == list(range(k)) == want["const"][0][0].tolist()
    for nq in tor.MANY_NQS:
        slices = HOOK(0, tor.SPARSE_V, n, nq, k, cases.SEG_DEFAULT)["n_slices"]
        assert slices >= 17 and (k != 256 or slices * k > tor.MERGE_OUTER)
        lay = tor.many_layout(nq)
        ixr.assert_same(many.search_inverted(*tor.sparse_query(lay), k), tor.of_layout(want, lay), (k, nq))


# ------------------------------------------------------------------------------------------------
# 7. which kernels this file ran
# ------------------------------------------------------------------------------------------------
def test_every_instantiation_of_the_inverted_scan_ran_under_this_file(model):
    """a small search per instantiation of its own (so that the test stands alone), then the profiler's launch counts, which after a run
    of the whole file hold every test above"""
    for dtype in tor.SPARSE_DTYPES:
        fx = tor.sparse_fixture(dtype, 128, "allow")
        ix = sparse_index(model, fx, "allow")
        invert(model, ix, 256)
        q = tor.sparse_query(fx.kinds)
        ixr.assert_same(ix.search_inverted(*q, 128), tor.of_layout({kk: tor.reference_topk(fx.scores[kk][None], True, 128) for kk in fx.kinds}, fx.kinds), dtype)
        ixr.assert_same(ix.search_inverted(*q, 128, allow=fx.ok), tor.of_layout(per_kind(fx, 128), fx.kinds), dtype)
        ix.close()
    rep = model.profile_report()
    names = [f"sparse_postings_scan_{d}{m}" for d in tor.SPARSE_DTYPES for m in ("", "_masked")] + ["sparse_query_sort", "topk_merge"]
    for name in names:
        print(f"{name}: {rep.get(name, {}).get('launches', 0)} launches")
    for name in names:
        assert rep.get(name, {}).get("launches", 0) >= 1, (name, sorted(rep))
