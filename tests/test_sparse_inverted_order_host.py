"""CPU proof that the cells of test_gpu_sparse_inverted_order.py reach what they are there for (tests/topk_order_reference.py
INVERTED_CELLS: the sparse fixtures under the launch geometries of sparse_postings_scan_kernel).  The geometry of every cell comes from
the plan the search itself uses (sparse_postings_geometry through bert_hip_test_sparse_postings_geometry), per chunk of 4096 queries;
the model (sliced_search: one walk per slice and tile, then the merge) never calls the library.  Asserted per cell: the tile, how many
segments a workgroup walks, the shorter last slice, the partial last segment, the second chunk, LDS beyond 64 KiB, and — wherever a
workgroup sees all rows — the exact fit (count == room, unsorted, then a whole step up to slot L - 1; fresh under a mask, stale without)
and its near miss.  The last tests show that the model can tell: a queue that sorts one row late, a queue forgotten at a segment edge and
accumulators that are not zeroed between segments each select something else than the order rule.  Every test prints what its cells
reached (pytest -s)."""
import numpy as np
import pytest

from bert_cpp_amd import pybert as libbert

import sparse_inverted_cases as cases
import test_topk_order_host as toh
import topk_order_reference as tor

HOOK = libbert.test_sparse_postings_geometry
STEP = tor.SPARSE_STEP


def plan(n_rows, nq, k, seg, qb=0, n_vocab=tor.SPARSE_V):
    """the chunks of a call and their geometries; the row type takes no part in the plan"""
    p = tor.postings_plan(HOOK, 0, n_rows, nq, k, seg, qb, n_vocab)
    assert p == tor.postings_plan(HOOK, 1, n_rows, nq, k, seg, qb, n_vocab)
    return p


def model_cell(fx, cell, ok, near_miss=False):
    """every layout of a cell through the model, chunk by chunk.  The tiles of a layout repeat (tor.inverted_period), so a chunk of
    thousands of queries is modelled by one period of its tiles under the geometry of the WHOLE chunk: a workgroup depends on its own
    tile and slice alone.  Returns the results of the first chunk by layout."""
    p = plan(fx.n, cell.nq, cell.k, cell.seg, cell.qb)
    tor.check_inverted_geometry(cell, fx.n, p)
    tile, out = p[0][2]["qb"], {}
    for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, cell.nq, tile).items():
        for c0, c, g in p:
            part = lay[c0:c0 + min(c, tor.inverted_period(fx.kinds, tile))]
            S = fx.S(part)
            res = tor.postings_search(S, ok, cell.k, g)
            what = (cell, name, c0, "near miss" if near_miss else "")
            toh.same(res, S, ok, cell.k, what)
            assert len(res["wgs"]) == g["n_slices"] * -(-len(part) // g["qb"])
            if c0:
                continue
            out[name] = res
            if "fit" not in cell.reach:
                continue
            assert g["n_slices"] == 1                                 # a workgroup that sees all rows: the fixture's schedule is its own
            if not near_miss:
                toh.check_tile_states(fx, name, part, res, g["qb"], g["L"], cell.k, STEP, cell.mode, what)
            elif name != "mixed" and name.split(":")[1] == "asc":
                for w in res["wgs"]:
                    assert w["near_miss"][part[w["q0"]:w["q0"] + g["qb"]].index("asc")], what
    return out


def fit_summary(cell, out):
    """over a cell's layouts: (an exact fit before the first sort, one behind a sort, a near miss, the largest slot written)"""
    wgs = [w for res in out.values() for w in res["wgs"]]
    return (any(w["fit_fresh"].any() for w in wgs), any(w["fit_stale"].any() for w in wgs), any(w["near_miss"].any() for w in wgs),
            max(w["max_slot"] for w in wgs))


# ------------------------------------------------------------------------------------------------
# the ordered cells: one segment, walked segments, tiles
# ------------------------------------------------------------------------------------------------
def test_the_table_holds_the_cells_of_the_issue():
    cells = tor.INVERTED_CELLS
    assert len({repr(c) for c in cells}) == len(cells)
    assert {(c.seg, c.nq) for c in tor.inverted_cells("walked")} == set(tor.INVERTED_WALKED)
    assert {c.k for c in tor.inverted_cells("one")} == set(tor.SPARSE_KS) and {c.nq for c in tor.inverted_cells("one")} == {1, 2, 3, 5}
    assert {c.qb for c in tor.inverted_cells("tiles")} == {1, 2, 3, 4, 8}
    assert {int(r[5:]) for c in cells for r in c.reach if r.startswith("tile=")} == {1, 2, 3, 4}
    for c in cells:
        # every cell in which one workgroup sees all rows claims the exact fit
        assert ("fit" in c.reach) == bool(c.reach & {"one_segment", "walks_all"}), c


def test_the_three_geometries_worked_out_by_hand():
    n = tor.SPARSE_ROWS
    for nq in (1, 2, 3, 5, 70):
        for k in tor.SPARSE_KS:
            (_, _, g), = plan(n, nq, k, 4096)
            assert (g["n_segs"], g["n_slices"], g["slice_segs"]) == (1, 1, 1), g
    for k in tor.INVERTED_WALKED_KS:
        (_, _, g), = plan(n, 4096, k, 256)
        assert (g["qb"], g["n_qtiles"], g["n_segs"], g["n_slices"], g["slice_segs"]) == (2, 2048, 16, 1, 16), g
        (_, _, g), = plan(n, 600, k, 256)
        assert (g["n_qtiles"], g["max_slices"], g["slice_segs"], g["n_slices"]) == (300, 7, 3, 6), g
        assert g["n_segs"] - 5 * g["slice_segs"] == 1 and n - 15 * 256 == 160          # the last slice: one partial segment of 160 rows
        first, second = plan(n, 4097, k, 256)
        assert first[2] == plan(n, 4096, k, 256)[0][2] and second[:2] == (4096, 1) and second[2]["n_slices"] == 16


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.SPARSE_KS)
def test_one_segment_cells_reach_their_states(k, mode):
    fxs = [tor.sparse_fixture(d, k, mode) for d in tor.SPARSE_DTYPES]
    fx = fxs[0]
    for kk in fx.kinds:                                              # (both row types: the same scores, so one model)
        assert np.array_equal(fxs[0].scores[kk].view(np.uint32), fxs[1].scores[kk].view(np.uint32))
    L = tor.sparse_L(k)
    for cell in tor.inverted_cells("one", k=k, mode=mode):
        out = model_cell(fx, cell, fx.permitted())
        fresh, stale, near, slot = fit_summary(cell, out)
        assert (fresh if mode != "plain" else stale) and slot == L - 1, (cell, fresh, stale, slot)
        if mode == "plain":
            assert near, cell                                        # (the "over" query of the same index)
        if mode == "allow":
            assert fit_summary(cell, model_cell(fx, cell, fx.ok1, near_miss=True))[2], cell
        print(f"{cell}: fit fresh {int(fresh)} stale {int(stale)} near miss {int(near)} largest slot {slot} of {L}")
    if mode != "plain":
        # fit_mask's near miss needs no second cell under removals: the queue cannot tell a removed row from a disallowed one
        assert not np.array_equal(fx.ok, fx.ok1)


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.INVERTED_WALKED_KS)
def test_walked_cells_reach_their_states(k, mode):
    fx = tor.sparse_fixture("f32", k, mode)
    L = tor.sparse_L(k)
    for cell in tor.inverted_cells("walked", k=k, mode=mode):
        out = model_cell(fx, cell, fx.permitted())
        p = plan(fx.n, cell.nq, k, cell.seg)
        g = p[0][2]
        line = f"{cell}: {g['n_qtiles']} tiles, {g['n_slices']} slice(s) of {g['slice_segs']} of {g['n_segs']} segments"
        if "fit" in cell.reach:
            fresh, stale, near, slot = fit_summary(cell, out)
            assert (fresh if mode != "plain" else stale) and slot == L - 1, (cell, fresh, stale, slot)
            assert near or mode != "plain", cell
            if mode == "allow":
                assert fit_summary(cell, model_cell(fx, cell, fx.ok1, near_miss=True))[2], cell
            # the steps of a workgroup that fall on a segment edge with a queue that is neither empty nor about to be sorted
            edges = g["slice_segs"] - 1
            assert edges == g["n_segs"] - 1 >= 3
            line += f"; fit fresh {int(fresh)} stale {int(stale)} near miss {int(near)} largest slot {slot} of {L}; {edges} edges walked"
        else:
            assert (g["slice_segs"], g["n_slices"]) == (3, 6) and all(w["steps"] in (3 * cell.seg // STEP, 1) for res in out.values() for w in res["wgs"])
        if len(p) == 2:
            line += f"; second chunk: {p[1][2]['n_slices']} slices of one segment"
        print(line)


@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("n", tor.INVERTED_TILES)
def test_tile_cells_reach_their_states(n, mode):
    k = tor.INVERTED_TILE_K
    fx = tor.sparse_fixture("f32", k, mode)
    for cell in tor.inverted_cells("tiles", qb=n, mode=mode):
        out = model_cell(fx, cell, fx.permitted())
        (_, _, g), = plan(fx.n, cell.nq, k, cell.seg, n)
        assert g["qb"] == min(n, 4, cell.nq) and (n <= 4 or g["qb"] == min(4, cell.nq))          # 8 aims for 4
        if cell.seg == 256:
            assert (g["n_slices"], g["slice_segs"]) == (16, 1), g   # few queries: a slice per segment, 16 lists a query for the merge
        print(f"{cell}: tile {g['qb']}, {g['n_qtiles']} tiles, {g['n_slices']} slices" +
              (f", fit {fit_summary(cell, out)}" if "fit" in cell.reach else ""))


# ------------------------------------------------------------------------------------------------
# large LDS and high row numbers
# ------------------------------------------------------------------------------------------------
def big_masks(n=tor.INVERTED_BIG_ROWS):
    """name -> the rows that qualify: all; 200 rows around the edge of the 16384-row segment gone; segment 0 alone"""
    gone = np.ones(n, bool)
    gone[tor.INVERTED_BIG_GONE] = False
    return {"all": np.ones(n, bool), "edge gone": gone, "first 16384": np.arange(n) < 16384}


@pytest.mark.parametrize("seg,k,tile", tor.INVERTED_BIG)
def test_large_segments_take_more_than_64_kib_and_clamp_the_tile(seg, k, tile):
    n = tor.INVERTED_BIG_ROWS
    per_query = seg * 4 + 256 * 8 + tor.sparse_L(k) * 8 + 8
    for nq in tor.INVERTED_BIG_NQS:
        (_, _, g), = plan(n, nq, k, seg, tor.INVERTED_BIG_QB)
        assert g["qb"] == min(tile, nq) and g["lds"] == g["qb"] * per_query, g
        assert g["n_segs"] == -(-n // seg) == g["n_slices"] and g["slice_segs"] == 1, g
        if nq >= tor.INVERTED_BIG_QB:
            assert g["lds"] > tor.INVERTED_LDS_STATIC, g
            # clamped below the 4 asked for exactly where one query more would not fit
            assert tile == min(tor.INVERTED_BIG_QB, (160 * 1024 - 256) // per_query), g
    assert tile * per_query == {(16384, 10): 143376, (16384, 256): 151568, (8192, 10): 155680, (8192, 256): 129048}[(seg, k)]
    for dtype in tor.SPARSE_DTYPES:
        _, w, sc = tor.big_inverted_rows(dtype)
        assert w.max() <= 65504 or dtype == "f32"
        for name, ok in big_masks().items():
            want = {kk: tor.reference_topk(sc[kk][None], ok, k) for kk in sc}
            last = np.flatnonzero(ok)[-1]
            if dtype == "f32":
                assert want["asc"][0][0, 0] == last
            assert want["desc"][0][0].tolist() == list(range(k)) == want["const"][0][0].tolist()
            if name == "first 16384":
                assert want["asc"][0][0].max() == 16383 and want["asc"][0][0].min() > 2047         # u16 row numbers beyond the default segment
            if name == "edge gone" and k == 256:
                assert (want["asc"][0][0] < 16384).sum() > 0 and (want["asc"][0][0] >= 16384).sum() > 0
            lay = tor.many_layout(max(tor.INVERTED_BIG_NQS))
            S = np.stack([sc[kk] for kk in lay])
            (_, _, g), = plan(n, len(lay), k, seg, tor.INVERTED_BIG_QB)
            toh.same(tor.postings_search(S, ok, k, g), S, ok, k, (seg, k, dtype, name))
    gone = tor.INVERTED_BIG_GONE
    assert len(gone) == 200 and gone[0] // 32 != 16383 // 32 and (gone < 16384).sum() == 100      # mask words on both sides of the edge


# ------------------------------------------------------------------------------------------------
# several segments per slice on random scores; many slices
# ------------------------------------------------------------------------------------------------
def test_the_random_case_cuts_slices_of_three_and_two_segments_and_starves_a_query():
    V, _, width = cases.CASES["a"][:3]
    rows, seg = cases.ROWS_SLICED, cases.SEG_TEST
    nq = cases.NQ * cases.TILING
    for k in (1, 10, 256):
        (_, _, g), = plan(rows, nq, k, seg, 0, V)
        assert (g["qb"], g["n_qtiles"], g["max_slices"], g["n_segs"], g["slice_segs"], g["n_slices"]) == (2, 525, 4, 11, 3, 4), g
        assert rows - 10 * seg == 130                                # slices of 3, 3, 3 and 2 segments, the last segment partial
    ids, _, q_ids, _ = cases.data("a", rows)
    # hits[q, sg]: the postings a query's walk meets in a segment
    hits = np.zeros((cases.NQ, g["n_segs"]), np.int64)
    for sg in range(g["n_segs"]):
        held = np.bincount(ids[sg * seg:(sg + 1) * seg][ids[sg * seg:(sg + 1) * seg] >= 0], minlength=V)
        for q in range(cases.NQ):
            hits[q, sg] = held[q_ids[q][q_ids[q] >= 0]].sum()
    terms = (q_ids >= 0).sum(axis=1)
    partner = np.arange(cases.NQ) ^ 1
    starved = (terms[:, None] > 0) & (hits == 0) & (hits[partner] > 0)
    print("queries with terms that meet no posting in a segment while their tile's other query does:", np.argwhere(starved).tolist()[:8])
    # query 4 asks for two ids that no row holds: its wave walks two empty lists in every segment, beside query 5, which meets postings in
    # every one; query 0 has no term at all, beside query 1
    assert terms[4] == len(cases.ABSENT) and starved[4].all() and hits[5].all() and terms[0] == 0 and hits[1].all()


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_many_slices_reach_a_second_merge_round_behind_the_inverted_scan(k):
    n = tor.MANY_SPARSE_ROWS
    sc = tor.many_scores(n)
    for nq in tor.MANY_NQS:
        (_, _, g), = plan(n, nq, k, cases.SEG_DEFAULT)
        assert g["n_slices"] == 17 == g["n_segs"] and g["slice_segs"] == 1 and (k != 256 or g["n_slices"] * k > tor.MERGE_OUTER), g
        lay = tor.many_layout(nq)
        S = np.stack([sc[kk] for kk in lay])
        res = tor.postings_search(S, True, k, g)
        toh.same(res, S, True, k, ("inverted", nq, k))
        toh.check_many(res, lay, k, 17, ("inverted", nq, k))
        print(tor.describe(f"inverted f32 {n} rows nq={nq} k={k}", res), "slices", res["slices"])


# ------------------------------------------------------------------------------------------------
# the model can tell
# ------------------------------------------------------------------------------------------------
def _ids(w):
    return np.where(w["ids"] == tor.SENT, -1, w["ids"])


def test_wrong_queues_and_stale_accumulators_select_something_else():
    """sensitivity, on the model alone (no kernel is made wrong here).  (1) A queue that sorts only above room + 1 loses a row of the near
    miss, plain ("over") and masked (ascending rows under ok1).  (2) A queue whose count goes back to 0 at every segment edge, unsorted —
    with segments of 256 rows every step is an edge — returns another top-k on the staircase and on all-equal scores.  (The model drops
    the whole queue; a kernel that only resets its count loses what the next pushes overwrite and sorts the rest in later.)  (3)
    Accumulators zeroed for a slice's first segment only: a row's score is then its own plus those of the rows at its place in the
    segments before it, and the top-k's ids or scores differ."""
    found = {"sorts one row late": [], "forgets the queue at an edge": [], "forgets it, on the first rows alone": [], "keeps the accumulators": []}

    def shows(s, ok, k, whole, **wrong):
        """the first n — all rows (whole), or any index of the first n rows, n a multiple of 256: an ascending pattern hides a lost row
        behind the better rows that follow it — at which the wrong queue and the order rule differ, or 0; the right queue never does"""
        ok = np.broadcast_to(np.asarray(ok, dtype=bool), s.shape)
        for n in [len(s)] if whole else list(range(STEP, len(s), STEP)) + [len(s)]:
            want = tor.reference_topk(s[None, :n], ok[:n], k)[0]
            assert np.array_equal(_ids(tor.walk(s[None, :n], np.arange(n), ok[:n], k, tor.sparse_L(k), STEP)), want)
            if not np.array_equal(_ids(tor.walk(s[None, :n], np.arange(n), ok[:n], k, tor.sparse_L(k), STEP, **wrong)), want):
                return n
        return 0

    for k in tor.SPARSE_KS:
        fx = tor.sparse_fixture("f32", k, "plain")
        mk = tor.sparse_fixture("f32", k, "allow")
        for name, at in (("over", shows(fx.scores["over"], True, k, False, slack=1)), ("masked", shows(mk.scores["asc"], mk.ok1, k, False, slack=1))):
            if at:
                found["sorts one row late"].append((k, name, at))
        for kind in ("stair", "asc", "const"):
            for seg in (256, 1024):
                if shows(fx.scores[kind], True, k, True, forget=seg // STEP):
                    found["forgets the queue at an edge"].append((k, kind, seg))
                at = shows(fx.scores[kind], True, k, False, forget=seg // STEP)
                if at:
                    found["forgets it, on the first rows alone"].append((k, kind, seg, at))
        for seg in (256, 1024):
            differs = []
            for kind in ("asc", "saw"):
                kept = fx.scores[kind].copy()
                for r0 in range(seg, fx.n, seg):
                    kept[r0:r0 + seg] += kept[r0 - seg:r0 - seg + len(kept[r0:r0 + seg])]
                got, want = tor.reference_topk(kept[None], True, k), tor.reference_topk(fx.scores[kind][None], True, k)
                differs.append(not np.array_equal(got[0], want[0]) or not np.array_equal(got[1], want[1]))
            if all(differs):
                found["keeps the accumulators"].append((k, seg))
    for what, where in found.items():
        print(f"{what}: disagrees at {where}")
    assert {(k, name) for k, name, _ in found["sorts one row late"]} == {(k, name) for k in tor.SPARSE_KS for name in ("over", "masked")}
    assert found["keeps the accumulators"] == [(k, seg) for k in tor.SPARSE_KS for seg in (256, 1024)]
    forgot, first = found["forgets the queue at an edge"], found["forgets it, on the first rows alone"]
    # Segments of 256 rows and k > 128 (room >= 511: a step of 256 pushes is not sorted, and the edge behind it forgets it — nothing is ever
    # sorted, so no threshold forms and the result is what the last steps pushed): the staircase shows it on all 4000 rows at k = 255 and
    # 256 and on its first 1536 rows at k = 129, all-equal scores at every such k.  k <= 128 (room < 256: a busy step is always sorted, an
    # edge finds the queue empty or holding rows that later ones beat) and segments of 1024 rows (an edge every fourth step: the rows it
    # forgets are beaten later) do not show it here; the walked cells therefore run k = 129 and 256 at segments of 256 rows.
    assert {(k, kind) for k, kind, _ in forgot} >= {(255, "stair"), (256, "stair"), (129, "const"), (255, "const"), (256, "const")}, forgot
    assert {k for k, kind, _, _ in first if kind == "stair"} == {129, 255, 256} and all(k > 128 and seg == 256 for k, _, seg, _ in first), first
