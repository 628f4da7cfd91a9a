"""CPU proof that the fixtures of test_gpu_topk_order.py, test_gpu_token_index_order.py, test_gpu_token_scan_forms.py and
test_gpu_hybrid_order.py reach the queue states they are built for (tests/topk_order_reference.py: the patterns and the host model of
the selecting kernels' queue).
The geometry comes from the hooks the searches themselves plan with (bert_hip_test_index_plan, bert_hip_test_sparse_scan_geometry[_qb];
the hybrid scan, sparse_hybrid_scan_kernel: bert_hip_test_hybrid_chunk for the chunks of a call and the scan's plan for each chunk); the
model never calls the library.  The hybrid section also proves the split fixtures exact and shows that neither term alone nor the
weights swapped selects what H selects, and that a reader of the dense scores with a wrong row or query index returns another result.  A fixture that stops reaching
its state — after a change of a list length, a step or a plan — fails here, not silently on the GPU.  Every test prints the reached
state of its fixtures (pytest -s)."""
import os
import re

import numpy as np
import pytest

from bert_cpp_amd import pybert as libbert

import topk_order_reference as tor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ["bert_hip_test_index_plan", "bert_hip_test_sparse_scan_geometry_qb"]


def same(res, S, ok, k, what):
    """the model selects what the order rule selects"""
    want = tor.reference_topk(S, ok, k)
    assert np.array_equal(res["ids"], want[0]) and np.array_equal(res["scores"].view(np.uint32), want[1].view(np.uint32)), what


# ------------------------------------------------------------------------------------------------
# the hooks, the values, the model on hand-made cases
# ------------------------------------------------------------------------------------------------
def test_hooks_are_declared_and_exported_by_the_test_library_only():
    text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    L, T = libbert.lib(), libbert.test_lib()
    for hook in HOOKS:
        assert re.search(r"BERT_API int32_t " + hook + r"\(", text) and hook in libbert.BERT_HIP_TEST_H_SYMBOLS
        assert hasattr(T, hook) and not hasattr(L, hook)


@pytest.mark.parametrize("args, want", [
    # (n_rows, nq, k)
    ((0, 1, 1), dict(nqt=1, slices=1, slice_rows=128, L=256)),
    ((2500, 33, 128), dict(nqt=2, slices=1, slice_rows=2560, L=256)),
    ((2500, 32, 129), dict(nqt=1, slices=1, slice_rows=2560, L=512)),
    ((17 * 4096, 33, 256), dict(nqt=2, slices=17, slice_rows=4096, L=512)),
    ((17 * 4096, 1, 10), dict(nqt=1, slices=34, slice_rows=2048, L=256)),
    ((1000000, 4096, 100), dict(nqt=128, slices=16, slice_rows=62592, L=256)),
])
def test_index_plan_table(args, want):
    assert libbert.test_index_plan(*args) == want


def test_index_plan_invariants_and_refusals():
    for k in (1, 127, 128, 129, 256):
        for nq in (1, 31, 32, 33, 4096):
            for n in (0, 1, 127, 128, 129, 2047, 2048, 4097, 2500, 69632, 1000000, 2 ** 31 - 1):
                g = libbert.test_index_plan(n, nq, k)
                assert g["nqt"] == -(-nq // 32) and g["L"] == tor.dense_L(k) and g["L"] - k - tor.DENSE_STEP >= 0
                assert g["slice_rows"] % tor.DENSE_STEP == 0 and g["slices"] >= 1
                assert g["slices"] * g["slice_rows"] >= n > (g["slices"] - 1) * g["slice_rows"] - (n == 0)
    P = libbert.test_index_plan
    assert P(-1, 1, 1) is None and P(10, 0, 1) is None and P(10, 4097, 1) is None and P(10, 1, 0) is None and P(10, 1, 257) is None
    assert libbert.test_lib().bert_hip_test_index_plan(10, 1, 1, None) == -1
    assert libbert.test_lib().bert_hip_test_sparse_scan_geometry_qb(0, 100, 10, 1, 1, 0, None) == -1


def test_values_are_exact_in_f16_and_ascending():
    v = tor.VALUES
    assert v[0] == 0 and (v[:2049] == np.arange(2049)).all() and (np.diff(v) > 0).all() and len(v) > 7000
    assert np.array_equal(v.astype(np.float16).astype(np.float32), v) and v[-1] == 65504


def test_the_model_on_hand_made_queues():
    # k = 2, L = 8, steps of 4: room = 2
    s = np.array([[1, 2, 3, 4, 0, 0, 5, 6, 7, 8, 9, 10]], np.float32)
    w = tor.walk(s, np.arange(12), True, 2, 8, 4)
    # step 0 pushes 4 > room: sort, threshold (3, 2); step 1 pushes 5, 6: count 2 == room, no sort; step 2 pushes 4: slots up to 2 + 5 = 7
    assert w["sort_steps"] == [0, 2] and w["max_slot"] == 7 and w["fit_stale"][0] and not w["fit_fresh"][0] and w["pushed_late"][0]
    assert w["ids"].tolist() == [[11, 10]] and w["scores"].tolist() == [[10.0, 9.0]]
    # all ties: only the first k rows ever push; a masked row never does
    w = tor.walk(np.zeros((1, 12), np.float32), np.arange(12), np.arange(12) != 0, 2, 8, 4)
    assert w["ids"].tolist() == [[1, 2]] and not w["pushed_late"][0] and w["sorts"] == 1 and w["max_slot"] == 4
    # two queries share the sort: the idle one's count is reset with the busy one's
    both = np.stack([s[0], -s[0]])
    w = tor.walk(both, np.arange(12), True, 2, 8, 4)
    assert w["ids"].tolist() == [[11, 10], [4, 5]] and w["pushed_late"].tolist() == [True, True]
    # fresh fit: two rows allowed, then a whole step, thresholds still -inf
    ok = np.ones(12, bool)
    ok[[1, 3]] = False
    w = tor.walk(s, np.arange(12), ok, 2, 8, 4)
    assert w["fit_fresh"][0] and w["max_slot"] == 7 and w["sort_steps"] == [1, 2]


def test_fit_schedule_counts():
    for step, Lf in ((tor.DENSE_STEP, tor.dense_L), (tor.SPARSE_STEP, tor.sparse_L)):
        for k in (1, 127, 128, 129, 255, 256):
            L = Lf(k)
            room = L - k - step
            push = tor.fit_schedule(20 * step, k, L, step, 0)
            steps = push.reshape(20, step).sum(axis=1)
            cyc = (room // step + (room % step > 0) if room else 1) + 1
            assert steps[:cyc - 1].sum() == room and steps[cyc - 1] == step and (steps[:cyc] == steps[cyc:2 * cyc]).all(), (step, k, steps)


# ------------------------------------------------------------------------------------------------
# index_topk_kernel
# ------------------------------------------------------------------------------------------------
def check_near_miss_mask(fx, nq, tile, k, L, step, plan):
    """the second allow-list of a masked fixture: one row more than fits while the thresholds are still -inf — sorted, then a whole step"""
    for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tile).items():
        S = fx.S(lay)
        res = tor.sliced_search(S, fx.ok1, k, tile, plan[0], plan[1], L, step)
        same(res, S, fx.ok1, k, (fx.name, "near miss", nq, name))
        for w in res["wgs"]:
            kinds = lay[w["q0"]:w["q0"] + tile]
            if name != "mixed" and name.split(":")[1] == "asc":
                pos = kinds.index("asc")
                assert w["near_miss"][pos], (fx.name, "near miss", nq, name)


def check_tile_states(fx, name, lay, res, tile, L, k, step, mode, what):
    """the states a first / last / mixed layout is built for, over the workgroups of res"""
    room = L - k - step
    for w in res["wgs"]:
        q0 = w["q0"]
        kinds = lay[q0:q0 + tile]
        if name == "mixed":
            if room == 0 and "asc" in kinds and fx.ok is None:
                assert w["sorts"] == w["steps"], (what, "a sort at every step", w["sorts"], w["steps"])
            continue
        b = name.split(":")[1]
        pos = [i for i, kk in enumerate(kinds) if kk == b]
        idle = [i for i, kk in enumerate(kinds) if kk != b]
        assert len(pos) == 1 and pos[0] == (0 if name.startswith("first") else len(kinds) - 1)
        # the idle neighbours never push after their first k rows
        assert not w["pushed_late"][idle].any(), (what, "idle neighbours")
        if b in ("asc", "stair"):
            assert w["pushed_late"][pos[0]], what
        if b == "stair":
            assert w["fit_stale"][pos[0]] and w["max_slot"] == L - 1, (what, "exact fit, stale thresholds", w["max_slot"])
        if b == "over":
            assert w["near_miss"][pos[0]], (what, "one row more than fits: sorted, then a whole step")
        if b == "asc" and mode != "plain":
            assert w["fit_fresh"][pos[0]] and w["max_slot"] == L - 1, (what, "exact fit, thresholds still -inf", w["max_slot"])
        if b == "asc" and mode == "plain" and room == 0:
            assert w["sorts"] == w["steps"] and w["max_slot"] == L - 1, (what, "a sort at every step")


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.DENSE_KS)
@pytest.mark.parametrize("dtype", tor.DENSE_DTYPES)
def test_dense_fixtures_reach_their_states(dtype, k, mode):
    for fx in tor.dense_fixtures(dtype, k, mode):
        for nq in tor.DENSE_NQS:
            g = libbert.test_index_plan(fx.n, nq, k)
            assert g["L"] == tor.dense_L(k) and g["slices"] == 1 and g["nqt"] == -(-nq // tor.QT), g
            assert 15 <= -(-fx.n // tor.DENSE_STEP) <= 20 and fx.n % tor.DENSE_STEP != 0
            for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tor.QT).items():
                S = fx.S(lay)
                res = tor.sliced_search(S, fx.permitted(), k, tor.QT, g["slices"], g["slice_rows"], g["L"], tor.DENSE_STEP)
                what = (fx.name, nq, name)
                same(res, S, fx.permitted(), k, what)
                check_tile_states(fx, name, lay, res, tor.QT, g["L"], k, tor.DENSE_STEP, mode, what)
                if nq == 32:
                    print(tor.describe(f"{fx.name} nq={nq} {name}", res))
            if mode == "allow":
                check_near_miss_mask(fx, nq, tor.QT, k, g["L"], tor.DENSE_STEP, (g["slices"], g["slice_rows"]))
        if mode != "plain":
            # the mask: some whole 32-row word is empty (k = 128) or not, and the masked kernel is the one launched
            assert not fx.ok.all() and fx.ok.sum() > 256


# ------------------------------------------------------------------------------------------------
# many slices: the merge
# ------------------------------------------------------------------------------------------------
def check_many(res, lay, k, slices_aimed, what):
    assert res["slices"] >= slices_aimed, what
    m = res["merge"]
    if k == 256:
        assert m["rounds"] >= 2 and m["n_cand"] == res["slices"] * k > tor.MERGE_OUTER, what
        for q, kind in enumerate(lay):
            w = m["walks"][q]
            if kind == "asc":
                # every slice beats all earlier ones: the merge takes a whole list per round, sorts after each, and fills its queue to the end
                assert w["sorts"] == res["slices"] and w["max_slot"] == tor.MERGE_L - 1, (what, w["sorts"])
            else:
                assert w["sorts"] == 1 and not w["pushed_late"][0], what


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_many_slices_reach_a_second_merge_round(k):
    n = tor.MANY_DENSE_ROWS
    sc = tor.many_scores(n)
    for nq in tor.MANY_NQS:
        lay = tor.many_layout(nq)
        S = np.stack([sc[kk] for kk in lay])
        g = libbert.test_index_plan(n, nq, k)
        res = tor.sliced_search(S, True, k, tor.QT, g["slices"], g["slice_rows"], g["L"], tor.DENSE_STEP)
        same(res, S, True, k, ("dense", nq, k))
        check_many(res, lay, k, 17, ("dense", nq, k))
        print(tor.describe(f"dense f32 {n} rows nq={nq} k={k}", res), "slices", res["slices"])
    n = tor.MANY_SPARSE_ROWS
    sc = tor.many_scores(n)
    for nq in tor.MANY_NQS:
        lay = tor.many_layout(nq)
        S = np.stack([sc[kk] for kk in lay])
        g = libbert.test_sparse_scan_geometry(0, tor.SPARSE_V, n, nq, k)
        assert g["L"] == tor.sparse_L(k)
        res = tor.sliced_search(S, True, k, g["qb"], g["n_slices"], g["slice_rows"], g["L"], tor.SPARSE_STEP)
        same(res, S, True, k, ("sparse", nq, k))
        check_many(res, lay, k, 17, ("sparse", nq, k))
        print(tor.describe(f"sparse f32 {n} rows nq={nq} k={k}", res), "slices", res["slices"])


@pytest.mark.parametrize("k", tor.MERGE_KS)
def test_rescored_candidates_reach_the_merge_s_exact_fit(k):
    sc = tor.merge_scores(k)
    S = np.stack([sc[kk] for kk in tor.MERGE_KINDS])
    m = tor.merge(S, np.tile(np.arange(tor.MERGE_CAND), (len(S), 1)), k)
    same(m, S, True, k, k)
    by = dict(zip(tor.MERGE_KINDS, m["walks"]))
    assert m["n_cand"] == tor.MERGE_CAND and by["stair"]["steps"] == 4
    assert by["stair"]["fit_stale"][0] and by["stair"]["max_slot"] == tor.MERGE_L - 1 and by["over"]["near_miss"][0]
    assert not by["const"]["pushed_late"][0]
    print(f"merge k={k}: " + ", ".join(f"{kk}: sorts {w['sorts']} largest slot {w['max_slot']} of {w['L']} (room {w['room']})" for kk, w in by.items()))


# ------------------------------------------------------------------------------------------------
# index_probe_kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tor.PROBE_FORMS)
@pytest.mark.parametrize("k", tor.PROBE_KS)
@pytest.mark.parametrize("dtype", tor.DENSE_DTYPES)
def test_probe_fixtures_reach_their_states(dtype, k, form):
    fx = tor.probe_fixture(dtype, k, form)
    masked = form == "allow"
    L = tor.dense_L(k)
    assert len(fx.long_rows) >= 1500 and fx.n - fx.n_part > tor.PROBE_CHUNK and fx.n_part % 32 != 0
    lay = tor.probe_layout()
    S = fx.S(lay)
    res = tor.probed_search(S, fx.permitted(), k, fx.lists, tor.PROBE_LISTS)
    same(res, S, fx.permitted(), k, fx.name)
    assert len(res["items"]) == tor.PROBE_LISTS + 2 and res["wgs"][3] is None          # an empty list; two tail chunks
    long_list = res["wgs"][0]
    if form == "over":
        assert long_list["near_miss"][0], fx.name
    else:
        assert long_list["max_slot"] == L - 1 and long_list["fit_fresh" if masked else "fit_stale"][0], (fx.name, long_list["max_slot"])
    assert not long_list["pushed_late"][2]                           # (the constant query)
    if masked:
        near = tor.probed_search(S, fx.ok1, k, fx.lists, tor.PROBE_LISTS)
        same(near, S, fx.ok1, k, (fx.name, "near miss"))
        assert near["wgs"][0]["near_miss"][0], fx.name
    if k == 128 and not masked:
        tail = res["wgs"][tor.PROBE_LISTS]
        assert tail["sorts"] == tail["steps"] == tor.PROBE_CHUNK // tor.DENSE_STEP         # ascending at room 0: a sort at every step
    print(tor.describe(fx.name, res))


# ------------------------------------------------------------------------------------------------
# sparse_index_scan_kernel
# ------------------------------------------------------------------------------------------------
SPARSE_NQS = (1, 2, 3, 5)


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.SPARSE_KS)
@pytest.mark.parametrize("dtype", tor.SPARSE_DTYPES)
def test_sparse_fixtures_reach_their_states(dtype, k, mode):
    fx = tor.sparse_fixture(dtype, k, mode)
    for nq in SPARSE_NQS:
        g = libbert.test_sparse_scan_geometry(tor.SPARSE_DTYPES.index(dtype), tor.SPARSE_V, fx.n, nq, k)
        assert g["L"] == tor.sparse_L(k) and g["n_slices"] == 1 and g["qb"] == min(2, nq), g
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, g["qb"]).items():
            S = fx.S(lay)
            res = tor.sliced_search(S, fx.permitted(), k, g["qb"], 1, g["slice_rows"], g["L"], tor.SPARSE_STEP)
            what = (fx.name, nq, name)
            same(res, S, fx.permitted(), k, what)
            check_tile_states(fx, name, lay, res, g["qb"], g["L"], k, tor.SPARSE_STEP, mode, what)
            if nq == 2:
                print(tor.describe(f"{fx.name} nq={nq} {name}", res))
        if mode == "allow":
            check_near_miss_mask(fx, nq, g["qb"], k, g["L"], tor.SPARSE_STEP, (1, g["slice_rows"]))
    if k == 256 and mode == "plain":
        # room 512: two whole steps behind a sort, unsorted, and a third up to slot 1023
        st = fx.scores["stair"]
        lead = tor.staircase_lead(k, 1024, tor.SPARSE_STEP)
        assert (st[lead * 256:(lead + 3) * 256] > 0).all() and g["L"] - k - tor.SPARSE_STEP == 512


TILES = (1, 2, 3, 4, 5, 8)


def tile_nqs(n):
    return sorted({n - 1, n, n + 1, 70} - {0})


@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("n", TILES)
def test_sparse_tile_sizes_reach_their_states(n, mode):
    k = 128
    fx = tor.sparse_fixture("f32", k, mode)
    for nq in tile_nqs(n):
        g = libbert.test_sparse_scan_geometry(0, tor.SPARSE_V, fx.n, nq, k, qb=n)
        assert g["qb"] == min(n, nq) and g["n_qtiles"] == -(-nq // g["qb"]), g
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, g["qb"]).items():
            S = fx.S(lay)
            res = tor.sliced_search(S, fx.permitted(), k, g["qb"], g["n_slices"], g["slice_rows"], g["L"], tor.SPARSE_STEP)
            same(res, S, fx.permitted(), k, (fx.name, n, nq, name))
            check_tile_states(fx, name, lay, res, g["qb"], g["L"], k, tor.SPARSE_STEP, mode, (fx.name, n, nq, name))
        print(tor.describe(f"{fx.name} tile {n} nq={nq} {name}", res))


def test_sparse_tile_option_values_and_the_lds_clamp():
    G = libbert.test_sparse_scan_geometry
    table = G(0, 30522, 5000, 70, 10)
    for bad in (0, 9, -1):
        assert G(0, 30522, 5000, 70, 10, qb=bad) == table
    assert G(0, 30522, 5000, 70, 10, qb=2) == table and table["qb"] == 2
    for n in TILES:
        assert G(1, 30522, 5000, 70, 10, qb=n)["qb"] == n
    # the largest query image: the LDS takes fewer than 8 of them
    for k, want in ((10, 3), (256, 2)):
        g = G(0, 262144, 130, 70, k, qb=8)
        assert 1 <= g["qb"] < 8 and g["qb"] == want and g["lds"] <= 160 * 1024 - 256 < g["lds"] // g["qb"] * (g["qb"] + 1), g


# ------------------------------------------------------------------------------------------------
# token_index_scan_kernel
# ------------------------------------------------------------------------------------------------
def test_staircase_lead_of_the_geometries_that_had_one_is_unchanged():
    """the generalised lead is, wherever the first sort already sees k rows, the closed form the dense, sparse and merge fixtures were built
    with; at the token scan's step of 64 it is the step after which a sort has left k rows"""
    geometries = [(k, tor.dense_L(k), tor.DENSE_STEP) for k in tor.DENSE_KS + tor.PROBE_KS]
    geometries += [(k, tor.sparse_L(k), tor.SPARSE_STEP) for k in tor.SPARSE_KS]
    geometries += [(k, tor.MERGE_L, tor.MERGE_STEP) for k in tor.MERGE_KS]
    for k, L, step in geometries:
        lead = (L - k - step) // step + 1
        assert lead * step >= k and tor.staircase_lead(k, L, step) == lead, (k, L, step)
    want = {1: 3, 64: 3, 128: 2, 129: 3, 191: 3, 192: 3, 193: 4, 255: 4, 256: 4}
    for k in tor.TOKEN_KS:
        L = tor.token_L(k)
        lead = tor.staircase_lead(k, L, tor.TOKEN_STEP)
        assert lead == want[k], (k, lead)
        # by the model: all rows push for `lead` steps; the last of them ends in a sort that leaves k rows, the one before does not
        w = tor.walk(tor.values(tor.ascending(lead * tor.TOKEN_STEP))[None], np.arange(lead * tor.TOKEN_STEP), True, k, L, tor.TOKEN_STEP)
        assert w["sort_steps"] and w["sort_steps"][-1] == lead - 1 and (w["ids"] != tor.SENT).all(), (k, w["sort_steps"])
        earlier = [t for t in w["sort_steps"] if t < lead - 1]
        assert not earlier or (earlier[-1] + 1) * tor.TOKEN_STEP < k, (k, w["sort_steps"])


def test_token_list_geometry_matches_the_library():
    for k in range(1, 257):
        L = tor.token_L(k)
        assert L == (256 if k <= 192 else 512) and L - k - tor.TOKEN_STEP >= 0
    rooms = {k: tor.token_L(k) - k - tor.TOKEN_STEP for k in tor.TOKEN_KS}
    assert rooms == {1: 191, 64: 128, 128: 64, 129: 63, 191: 1, 192: 0, 193: 255, 255: 193, 256: 192}
    text = open(os.path.join(ROOT, "bert.cpp_amd", "csrc", "token_index_kernels.h")).read()
    assert "constexpr int TOKEN_ROUNDS = 16;" in text and "TOKEN_STEP_DOCS = NWAVE * TOKEN_ROUNDS" in text
    assert "inline int token_list_L(int k) { return k + TOKEN_STEP_DOCS <= 256 ? 256 : 512; }" in text
    assert tor.MERGE_OUTER == 4096 and tor.TOKEN_STEP == 4 * 16


# the largest slot the ascending pattern writes in one slice of TOKEN_DOCS documents (the state the fixture was designed to: a change of
# the step, the list rule or the document count shows here)
TOKEN_ASC_SLOT = {1: 192, 64: 255, 128: 255, 129: 192, 191: 254, 192: 255, 193: 448, 255: 510, 256: 511}


@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_token_fixtures_reach_their_states(k):
    import token_index_reference as tref

    fx = tor.token_fixture(k)
    L = tor.token_L(k)
    room = L - k - tor.TOKEN_STEP
    assert fx.n == tor.TOKEN_DOCS == 1573 and fx.n % tor.TOKEN_STEP == 37 and fx.n % 4 != 0
    assert sorted(set(fx.lens.tolist())) == sorted(tor.TOKEN_DOC_LENS) and fx.cu[-1] == len(fx.rows)
    kinds, lens = tor.token_layout()
    # the closed-form scores are the definition's, from the rows and the queries themselves, at both query lengths
    f64 = tor.token_scores_f64(fx, kinds, lens)
    for i, kk in enumerate(kinds):
        assert np.array_equal(f64[i], fx.scores[kk].astype(np.float64)), (k, kk, lens[i])
    assert (fx.scores["desc"] < 0).all() and (fx.scores["was"] < 0).all()          # an unmasked slot (0) would beat every one
    S = np.stack([fx.scores[kk] for kk in tor.TOKEN_KINDS])
    # one slice: the long walk
    res = tor.token_search(S, k, 1, fx.n)
    same(res, S, True, k, (fx.name, "one slice"))
    by = {kk: res["wgs"][i] for i, kk in enumerate(tor.TOKEN_KINDS)}
    for kk, w in by.items():
        assert w["max_slot"] < L and w["steps"] == 25 and w["room"] == room, (k, kk, w["max_slot"])
    assert by["stair"]["max_slot"] == L - 1 and by["stair"]["fit_stale"][0], (k, "exact fit, stale threshold", by["stair"]["max_slot"])
    assert by["over"]["near_miss"][0], (k, "one document more than fits: sorted, then a whole step")
    assert by["asc"]["max_slot"] == TOKEN_ASC_SLOT[k] and by["asc"]["pushed_late"][0], (k, by["asc"]["max_slot"])
    # all ties, and every document worse than the one before: the first k ids, and nothing pushes once a sort has left k rows
    lead = tor.staircase_lead(k, L, tor.TOKEN_STEP)
    for kk in ("const", "desc"):
        assert by[kk]["ids"][0].tolist() == list(range(k)) and (not by[kk]["sort_steps"] or by[kk]["sort_steps"][-1] < lead), (k, kk)
    if room == 0:
        assert by["asc"]["sorts"] == by["asc"]["steps"] and by["asc"]["sort_steps"] == list(range(25)), (k, "a sort at every step")
    if k in (64, 128, 256):
        assert by["asc"]["fit_fresh"][0] and by["asc"]["fit_stale"][0], k
    print(tor.describe(f"{fx.name} one slice", res))
    print(f"{fx.name}: " + ", ".join(f"{kk}: sorts {w['sorts']} largest slot {w['max_slot']}" for kk, w in by.items()))
    # the planned cut: slices that are no whole steps
    n_slices, slice_docs = libbert.test_token_index_plan(fx.n, len(kinds), 0)
    assert (n_slices, slice_docs) == tref.plan(fx.n, len(kinds)) and slice_docs % 4 != 0 and n_slices > 17
    planned = tor.token_search(S, k, n_slices, slice_docs)
    same(planned, S, True, k, (fx.name, "planned"))
    assert max(w["max_slot"] for w in planned["wgs"]) < L


def test_token_many_slices_reach_a_second_merge_round():
    k, n = tor.TOKEN_MANY_K, tor.TOKEN_MANY_DOCS
    fx = tor.token_fixture(k, n)
    n_slices, slice_docs = libbert.test_token_index_plan(n, 2 * len(tor.TOKEN_KINDS), tor.TOKEN_MANY_SLICES)
    assert n_slices == tor.TOKEN_MANY_SLICES == 17
    # slices end inside a step and inside a group of four waves, the last one too
    last = n - (n_slices - 1) * slice_docs
    assert slice_docs % tor.TOKEN_STEP != 0 and slice_docs % 4 != 0 and last % tor.TOKEN_STEP != 0 and last % 4 != 0
    S = np.stack([fx.scores[kk] for kk in tor.TOKEN_KINDS])
    res = tor.token_search(S, k, n_slices, slice_docs)
    same(res, S, True, k, fx.name)
    m = res["merge"]
    assert m["n_cand"] == 17 * 256 == 4352 > tor.MERGE_OUTER and m["rounds"] == 2
    asc = m["walks"][tor.TOKEN_KINDS.index("asc")]
    assert asc["pushed_late"][0] and asc["sorts"] >= 2                 # every slice beats the ones before: the merge refills
    print(tor.describe(fx.name, res))


# ------------------------------------------------------------------------------------------------
# token_index_scan_kernel: the int8 form, the masked and the listed instantiations
# ------------------------------------------------------------------------------------------------
def _one_slice(fx, kind, k, ok=True):
    """the single-slice walk of one kind of a token fixture"""
    return tor.token_search(fx.scores[kind][None], k, 1, fx.n, ok)


def test_int8_token_fixtures_keep_the_ranks_order_at_every_sign_and_length():
    """a quantised row keeps its one nonzero column exactly: score[a] < score[b] iff rank[a] < rank[b], equal iff equal, for every
    pattern, both signs and both query lengths (asserted when a fixture is made; restated here on the raw scores), the expected bits
    being token_i8_reference.scores_i8 of the rows"""
    import token_i8_reference as t8

    for k in tor.TOKEN_KS:
        for pattern in tor.TOKEN_I8_PATTERNS:
            fx = tor.token_i8_fixture(pattern, k)
            assert fx.n == tor.TOKEN_DOCS and sorted(set(fx.lens.tolist())) == sorted(tor.TOKEN_DOC_LENS) and fx.cu[-1] == len(fx.rows)
            assert (np.count_nonzero(fx.rows, axis=1) <= 1).all() and not fx.rows[:, 1:].any()
            r = fx.ranks
            for kk, sign in ((fx.pos, 1), (fx.neg, -1)):
                s = fx.scores[kk].astype(np.float64) * sign
                order = np.argsort(r, kind="stable")
                assert ((np.diff(s[order]) > 0) == (np.diff(r[order]) > 0)).all() and ((np.diff(s[order]) == 0) == (np.diff(r[order]) == 0)).all(), (fx.name, kk)
            assert (fx.scores[fx.neg][r > 0] < 0).all() and (fx.scores["const"] == 0).all()
    fx = tor.token_i8_fixture("asc")
    kinds, lens = tor.token_i8_layout(fx)
    q, qcu = tor.token_i8_queries(kinds, lens)
    sc = t8.scores_i8(q, qcu, fx.rows, fx.cu)
    for i, kk in enumerate(kinds):
        assert np.array_equal(sc[i].view(np.uint32), fx.scores[kk].view(np.uint32)), (kk, lens[i])
    # (not relied on: the scores are the integers themselves, but for a few that lie one ulp above — two roundings by the scales)
    exact = fx.scores["asc"] == tor.values(fx.ranks)
    assert np.array_equal(np.rint(fx.scores["asc"]), tor.values(fx.ranks))
    print(f"{fx.name}: {int(exact.sum())} of {fx.n} ascending scores are the integers themselves, the others within {float(np.abs(fx.scores['asc'] - tor.values(fx.ranks)).max()):.1e}")


@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_int8_token_fixtures_reach_their_states(k):
    L = tor.token_L(k)
    room = L - k - tor.TOKEN_STEP
    by = {}
    for pattern in tor.TOKEN_I8_PATTERNS:
        fx = tor.token_i8_fixture(pattern, k)
        S = np.stack([fx.scores[kk] for kk in fx.kinds])
        res = tor.token_search(S, k, 1, fx.n)
        same(res, S, True, k, (fx.name, "one slice"))
        for kk, w in zip(fx.kinds, res["wgs"]):
            by[(pattern, kk)] = w
            assert w["max_slot"] < L and w["steps"] == 25 and w["room"] == room
        print(tor.describe(f"{fx.name}, one slice at k={k}", res))
        n_slices, slice_docs = libbert.test_token_index_plan(fx.n, 2 * len(fx.kinds), 0)
        assert slice_docs == 17 and n_slices > 17
        same(tor.token_search(S, k, n_slices, slice_docs), S, True, k, (fx.name, "planned"))
    stair, over, asc = by[("stair", "stair")], by[("over", "over")], by[("asc", "asc")]
    assert stair["max_slot"] == L - 1 and stair["fit_stale"][0], (k, "exact fit, stale threshold", stair["max_slot"])
    assert over["near_miss"][0], (k, "one document more than fits: sorted, then a whole step")
    assert asc["max_slot"] == TOKEN_ASC_SLOT[k] and asc["pushed_late"][0]
    if room == 0:
        assert asc["sorts"] == asc["steps"] and asc["sort_steps"] == list(range(25)), (k, "a sort at every step")
    # all ties (const), and every document worse than the one before (desc): the first k ids
    for key in [(pattern, "const") for pattern in tor.TOKEN_I8_PATTERNS] + [("asc", "desc")]:
        assert by[key]["ids"][0].tolist() == list(range(k)), (k, key)


def test_int8_token_many_slices_reach_a_second_merge_round():
    k, n = tor.TOKEN_MANY_K, tor.TOKEN_MANY_DOCS
    fx = tor.token_i8_fixture("asc", n=n)
    n_slices, slice_docs = libbert.test_token_index_plan(n, 2 * len(fx.kinds), tor.TOKEN_MANY_SLICES)
    assert n_slices == 17 and slice_docs % tor.TOKEN_STEP != 0 and slice_docs % 4 != 0
    S = np.stack([fx.scores[kk] for kk in fx.kinds])
    res = tor.token_search(S, k, n_slices, slice_docs)
    same(res, S, True, k, fx.name)
    m = res["merge"]
    assert m["n_cand"] == 4352 > tor.MERGE_OUTER and m["rounds"] == 2 and m["walks"][0]["pushed_late"][0] and m["walks"][0]["sorts"] >= 2
    print(tor.describe(fx.name, res))


@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_masked_token_fixtures_reach_their_states(k):
    """fit_mask over the ascending pattern, for the f16 and the int8 fixture alike (both are ascending under "asc"): the exact fit while
    the threshold is still -inf, the near miss, steps without a qualifying document, slices that start inside a mask word"""
    L = tor.token_L(k)
    room = L - k - tor.TOKEN_STEP
    ok, ok1 = tor.token_masks(k)
    assert not ok.all() and not ok1.all() and ok.sum() > 256 and not np.array_equal(ok, ok1)
    for fx in (tor.token_fixture(k), tor.token_i8_fixture("asc")):
        S = np.stack([fx.scores[kk] for kk in tor.TOKEN_MASK_KINDS])
        for mask, name in ((ok, "exact fit"), (ok1, "near miss")):
            res = tor.token_search(S, k, 1, fx.n, mask)
            same(res, S, mask, k, (fx.name, name, "one slice"))
            asc = res["wgs"][0]
            if name == "exact fit":
                assert asc["max_slot"] == L - 1 and asc["fit_fresh"][0], (fx.name, k, "exact fit, threshold still -inf", asc["max_slot"])
            else:
                assert asc["near_miss"][0], (fx.name, k, "one document more than fits")
            print(tor.describe(f"{fx.name} masked k={k} {name} one slice", res))
            for slices in (0, 7):
                n_slices, slice_docs = libbert.test_token_index_plan(fx.n, 2 * len(tor.TOKEN_MASK_KINDS), slices)
                assert slice_docs == (17 if slices == 0 else 225)
                # the three-word mask: a slice, and so every step of it, starts inside a word
                assert any((s * slice_docs) & 31 for s in range(n_slices)), (slices, slice_docs)
                cut = tor.token_search(S, k, n_slices, slice_docs, mask)
                same(cut, S, mask, k, (fx.name, name, slices))
                assert max(w["max_slot"] for w in cut["wgs"]) < L
    if room == 0:
        # the kernel's `m == 0` skip: whole 64-aligned steps of the single-slice walk without a qualifying document
        steps = [ok[b:b + tor.TOKEN_STEP] for b in range(0, len(ok), tor.TOKEN_STEP)]
        assert sum(not s.any() for s in steps) >= 1 and any(s.all() for s in steps)
    for mode in tor.TOKEN_MASK_MODES:
        for mask in (ok, ok1):
            removed, allow = tor.token_mask_mode(mask, mode)
            assert (mode == "allow") == (len(removed) == 0) and (mode == "removed") == (allow is None)
            if mode == "both":
                assert 0 < len(removed) < (~mask).sum() and not allow.all()


def _same_listed(res, S, cand, removed, k):
    import token_index_reference as tref

    want = tref.rescore_expected(tor.list_scores(S, cand, removed), np.tile(cand, (len(S), 1)), k)
    return np.array_equal(res["ids"], want[0]) and np.array_equal(res["scores"].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_listed_fixtures_reach_their_states(k):
    """one slice of 1024 positions is 16 steps: the exact fit (fresh through the holes, stale through the staircase of ids) and both near
    misses for every k; the planned rescore's 64 slices of 16 positions reach the merge's second round at k = 256"""
    L = tor.token_L(k)
    fx = tor.listed_fixture()
    assert fx.n == tor.LIST_DOCS == 1024 and fx.scores["asc"][0] == 0 and (np.diff(fx.scores["asc"]) > 0).all()
    S = np.stack([fx.scores[kk] for kk in fx.kinds])
    lists = tor.candidate_lists(k)
    assert tor.staircase_lead(k, L, tor.TOKEN_STEP) + 5 <= 16
    state = {}
    for name, (cand, removed) in lists.items():
        valid = tor.list_valid(cand, removed)
        res = tor.listed_search(S, cand, valid, k, 1, len(cand))
        assert _same_listed(res, S, cand, removed, k), (k, name, "one slice")
        state[name] = res["wgs"][0]                                                  # (the "asc" query)
        assert res["wgs"][0]["steps"] == 16
        print(tor.describe(f"listed k={k} {name} one slice", res))
        n_slices, slice_pos = libbert.test_token_index_plan(len(cand), len(S), 0)
        assert (n_slices, slice_pos) == (64, 16)
        planned = tor.listed_search(S, cand, valid, k, n_slices, slice_pos)
        assert _same_listed(planned, S, cand, removed, k), (k, name, "planned")
        assert planned["merge"]["n_cand"] == 64 * k
        if k == 256:
            assert planned["merge"]["n_cand"] > tor.MERGE_OUTER and planned["merge"]["rounds"] >= 2
    assert state["holes"]["max_slot"] == L - 1 and state["holes"]["fit_fresh"][0], (k, state["holes"]["max_slot"])
    assert state["holes over"]["near_miss"][0], k
    assert state["repeats"]["max_slot"] == L - 1 and state["repeats"]["fit_stale"][0], (k, state["repeats"]["max_slot"])
    assert state["repeats over"]["near_miss"][0], k
    # the holes are of all four kinds, and a removed id is a document that would have been pushed
    cand, removed = lists["holes"]
    assert (cand == -1).any() and (cand == tor.LIST_DOCS).any() and (cand == 2 ** 31 - 1).any() and len(removed) > 0 and (cand[removed] == removed).all()
    # reversed: position order and id order disagree; repeats: document 0 is returned as often as it is named
    cand, _ = lists["reversed"]
    assert (np.diff(cand) < 0).all() and (np.diff(fx.scores["desc"][cand]) > 0).all()
    cand, removed = lists["repeats"]
    res = tor.listed_search(S, cand, tor.list_valid(cand, removed), k, 1, len(cand))
    zeros = int((cand == 0).sum())
    assert zeros > 1 and (res["ids"][1][:min(k, zeros)] == 0).all() and (k <= zeros or res["ids"][1][zeros] == 1)


def test_wrong_models_disagree_with_the_order_rule():
    """sensitivity, on the model alone: each deliberately wrong queue gives another result than the order rule on a new fixture (the
    right one agrees on all of them, above).  No kernel is made wrong for this."""
    fx = tor.listed_fixture()
    S = np.stack([fx.scores[kk] for kk in fx.kinds])
    found = {"a hole is pushed": [], "sorts only above room + 1": [], "positions for ids": []}
    for k in tor.TOKEN_KS:
        lists = tor.candidate_lists(k)
        n = tor.LIST_DOCS
        cand, removed = lists["holes"]
        if not _same_listed(tor.listed_search(S, cand, np.ones(n, bool), k, 1, n), S, cand, removed, k):
            found["a hole is pushed"].append(k)
        for name in ("holes over", "repeats over"):
            cand, removed = lists[name]
            late = tor.listed_search(S, cand, tor.list_valid(cand, removed), k, 1, n, slack=1)
            if not _same_listed(late, S, cand, removed, k):
                found["sorts only above room + 1"].append((k, name))
        cand, removed = lists["reversed"]
        if not _same_listed(tor.listed_search(S, cand, tor.list_valid(cand, removed), k, 1, n, positions_for_ids=True), S, cand, removed, k):
            found["positions for ids"].append(k)
        # the same queue over documents: the int8 near miss and the masked near miss
        over = tor.token_i8_fixture("over", k)
        w = tor.walk(over.scores["over"][None], np.arange(over.n), True, k, tor.token_L(k), tor.TOKEN_STEP, slack=1)
        want = tor.reference_topk(over.scores["over"][None], True, k)
        if not np.array_equal(np.where(w["ids"] == tor.SENT, -1, w["ids"]), want[0]):
            found["sorts only above room + 1"].append((k, "int8 over"))
        asc, ok1 = tor.token_i8_fixture("asc"), tor.token_masks(k)[1]
        w = tor.walk(asc.scores["asc"][None], np.arange(asc.n), ok1, k, tor.token_L(k), tor.TOKEN_STEP, slack=1)
        if not np.array_equal(np.where(w["ids"] == tor.SENT, -1, w["ids"]), tor.reference_topk(asc.scores["asc"][None], ok1, k)[0]):
            found["sorts only above room + 1"].append((k, "masked near miss"))
    for what, where in found.items():
        print(f"{what}: disagrees at {where}")
        assert where, what
    assert found["a hole is pushed"] == list(tor.TOKEN_KS) and found["positions for ids"] == list(tor.TOKEN_KS)
    # (k = 1: the one document the late sort loses is overtaken by a later one of the rising pattern, so the end result cannot show it)
    assert {k for k, _ in found["sorts only above room + 1"]} >= set(tor.TOKEN_KS) - {1}


# ------------------------------------------------------------------------------------------------
# sparse_hybrid_scan_kernel: the hybrid search's second pass
# ------------------------------------------------------------------------------------------------
_PLANNED = {}


def planned_search(H, ok, k, g):
    """sliced_search under a plan of the hook, made once per (scores, mask, plan): the weight pairs and the two sparse forms of a cell
    give the same H"""
    ok = np.ascontiguousarray(np.broadcast_to(np.asarray(ok, dtype=bool), H.shape[1:]))
    key = (H.tobytes(), ok.tobytes(), k, g["qb"], g["n_slices"], g["slice_rows"], g["L"])
    if key not in _PLANNED:
        _PLANNED[key] = tor.sliced_search(H, ok, k, g["qb"], g["n_slices"], g["slice_rows"], g["L"], tor.SPARSE_STEP)
    return _PLANNED[key]


def hybrid_tile(fx, nq, k, pref=0):
    """the scan's tile of a call's first chunk — every chunk but a last short one has it —, for layouts()"""
    chunks, _ = tor.hybrid_chunks(fx.n, nq, pref, libbert.test_hybrid_chunk)
    return libbert.test_sparse_scan_geometry(tor.SPARSE_DTYPES.index(fx.sd), tor.SPARSE_V, fx.n, chunks[0][1], k)["qb"]


def hybrid_model(fx, lay, ok, k, pref=0, want=None, what=""):
    """One call of the hybrid search as the library plans it: the chunks of bert_hip_test_hybrid_chunk, for each the scan's plan of
    bert_hip_test_sparse_scan_geometry, the model's walk over the reference's H.  Asserts that the model selects what
    hybrid_reference.search selects, bit for bit.  Returns [(c0, c, plan, walks)]."""
    chunks, ld = tor.hybrid_chunks(fx.n, len(lay), pref, libbert.test_hybrid_chunk)
    H = fx.S(lay)
    parts = []
    for c0, c in chunks:
        g = libbert.test_sparse_scan_geometry(tor.SPARSE_DTYPES.index(fx.sd), tor.SPARSE_V, fx.n, c, k)
        assert g["L"] == tor.sparse_L(k) and g["qb"] == min(2, c) and g["n_qtiles"] == -(-c // g["qb"]), g
        assert c0 % 2 == 0                                           # a chunk starts at a tile's first query: the layouts hold in every chunk
        parts.append((c0, c, g, planned_search(H[c0:c0 + c], ok, k, g)))
    want = tor.of_layout(tor.hybrid_reference(fx, k, ok), lay) if want is None else want
    ids = np.concatenate([p[3]["ids"] for p in parts])
    sc = np.concatenate([p[3]["scores"] for p in parts])
    assert np.array_equal(ids, want[0]) and np.array_equal(sc.view(np.uint32), want[1].view(np.uint32)), what
    return parts


def check_hybrid_states(fx, name, lay, parts, k, near, what):
    """check_tile_states over every chunk, the kinds named by what H does (a negative weight pair makes "desc" the ascending one), and what
    the walks of §1's table reach beyond it.  near: the mask is the near miss's (ok1)."""
    L = tor.sparse_L(k)
    eff = name if name == "mixed" else name.split(":")[0] + ":" + fx.effective[name.split(":")[1]]
    for c0, c, g, res in parts:
        kinds = [fx.effective[kk] for kk in lay[c0:c0 + c]]
        if near:
            for w in res["wgs"]:
                if eff.endswith(":asc"):
                    pos = kinds[w["q0"]:w["q0"] + g["qb"]].index("asc")
                    assert w["near_miss"][pos], (what, "one row more than fits while the thresholds are -inf")
            continue
        check_tile_states(fx, eff, kinds, res, g["qb"], L, k, tor.SPARSE_STEP, fx.mode, what)
        if eff == "mixed":
            continue
        b = eff.split(":")[1]
        for w in res["wgs"]:
            pos = kinds[w["q0"]:w["q0"] + g["qb"]].index(b)
            assert w["max_slot"] < L
            if b == "stair":
                assert w["fit_fresh"][pos] == (k == 256), (what, "k = 256: the lead itself fits exactly, before the first sort")
            if b == "asc" and fx.mode != "plain":
                assert w["fit_stale"][pos] == tor.masked_reaches_stale(fx.n, k), (what, "the second exact fit, behind a sort")


def hybrid_cell(fx, k, nqs, pref=0, show=None):
    """every layout of every nq of one index pair: the result, the states, and (allow) the near miss of the same pair"""
    for nq in nqs:
        tile = hybrid_tile(fx, nq, k, pref)
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tile).items():
            what = (fx.name, nq, name)
            parts = hybrid_model(fx, lay, fx.permitted(), k, pref, what=what)
            check_hybrid_states(fx, name, lay, parts, k, False, what)
            if nq == show:
                print(tor.describe(f"{fx.name} nq={nq} {name}", parts[0][3]))
            if fx.mode == "allow":
                parts = hybrid_model(fx, lay, fx.ok1, k, pref, what=(*what, "near miss"))
                check_hybrid_states(fx, name, lay, parts, k, True, (*what, "near miss"))


def test_hybrid_schedules_reach_what_the_walks_of_one_query_reach():
    """the staircase and fit_mask at step 256 and L = sparse_L(k), one query, one slice, every k at both sizes"""
    for n in sorted(set(tor.HYBRID_ROWS.values())):
        for k in tor.HYBRID_KS:
            L = tor.sparse_L(k)
            ids = np.arange(n)
            st = tor.walk(tor.values(tor.staircase(n, k, L, tor.SPARSE_STEP))[None], ids, True, k, L, tor.SPARSE_STEP)
            assert st["max_slot"] == L - 1 and st["fit_stale"][0] and st["fit_fresh"][0] == (k == 256), (n, k)
            ov = tor.walk(tor.values(tor.staircase(n, k, L, tor.SPARSE_STEP, 1))[None], ids, True, k, L, tor.SPARSE_STEP)
            assert ov["near_miss"][0], (n, k)
            asc = tor.values(tor.ascending(n))[None]
            mk = tor.walk(asc, ids, tor.fit_mask(n, k, L, tor.SPARSE_STEP), k, L, tor.SPARSE_STEP)
            assert mk["max_slot"] == L - 1 and mk["fit_fresh"][0] and mk["fit_stale"][0] == tor.masked_reaches_stale(n, k), (n, k)
            assert tor.walk(asc, ids, tor.fit_mask(n, k, L, tor.SPARSE_STEP, 1), k, L, tor.SPARSE_STEP)["near_miss"][0], (n, k)
    assert tor.SPARSE_ROWS == 15 * 256 + 160 and tor.HYBRID_ROWS["b1"] == 7 * 256 + 248
    assert libbert.test_hybrid_chunk(tor.SPARSE_ROWS, 1)[1] == 4032 and 4032 - tor.SPARSE_ROWS < 64          # a partial last block of 64


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.HYBRID_KS)
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
def test_hybrid_split_fixtures_reach_their_states(sd, k, mode):
    for w in tor.HYBRID_WEIGHTS:
        fx = tor.hybrid_split_fixture(sd, sd, k, mode, w)
        assert fx.n == tor.SPARSE_ROWS and fx.busy[-1] == ("asc" if w[0] > 0 else "desc")                    # a negative pair: desc rises
        hybrid_cell(fx, k, tor.HYBRID_NQS, show=2 if w == (1.0, 1.0) else None)
        if mode == "removed":
            for three_ways in (True, False):
                gone_d, gone_s, allow = tor.hybrid_removed_split(fx.ok, three_ways)
                assert three_ways == (len(gone_d) > 0) == (allow is not None) and len(gone_s) > 0
                assert not three_ways or k == 256 or not allow.all()


@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("k", tor.HYBRID_DENSE_KS)
@pytest.mark.parametrize("dd", tor.DENSE_DTYPES)
def test_hybrid_dense_carriers_reach_their_states(dd, k, mode):
    fxs = tor.hybrid_dense_fixtures(dd, "f32", k, mode)
    assert len(fxs) == (1 if dd in ("f32", "f16") else 4 if mode == "plain" else 2)
    assert libbert.test_hybrid_chunk(tor.HYBRID_ROWS[dd], 33) == (32, 4032 if dd != "b1" else 2048)          # 33 queries: chunks of 32 + 1
    for fx in fxs:
        assert fx.n == tor.HYBRID_ROWS[dd] and fx.rows.shape == (fx.n, tor.B1_DIM if dd == "b1" else tor.FLOAT_DIM)
        hybrid_cell(fx, k, tor.HYBRID_DENSE_NQS, show=33)


@pytest.mark.parametrize("k", tor.HYBRID_SPARSE_KS)
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
@pytest.mark.parametrize("dd", ["f32", "f16"])
def test_hybrid_sparse_carriers_reach_their_states(dd, sd, k):
    fx = tor.hybrid_sparse_fixture(dd, sd, k)
    assert fx.rows.any() and all(not q.any() for q in fx.dense_q.values())                                   # the rows are not zero: the query is
    hybrid_cell(fx, k, tor.HYBRID_NQS, show=2)


@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
def test_hybrid_chunked_fixtures_reach_their_states(sd, mode):
    k, nq, pref = tor.HYBRID_CHUNK_K, tor.HYBRID_CHUNK_NQ, tor.HYBRID_CHUNK
    assert libbert.test_hybrid_chunk(tor.SPARSE_ROWS, nq, pref) == (2, 4032)
    assert tor.hybrid_chunks(tor.SPARSE_ROWS, nq, pref, libbert.test_hybrid_chunk)[0] == [(0, 2), (2, 2), (4, 1)]
    for w in tor.HYBRID_WEIGHTS:
        hybrid_cell(tor.hybrid_split_fixture(sd, sd, k, mode, w), k, (nq,), pref=pref, show=nq if w == (1.0, 1.0) else None)


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_hybrid_many_slices_reach_a_second_merge_round(k):
    fx = tor.many_hybrid_fixture()
    assert fx.n == tor.MANY_SPARSE_ROWS and (fx.rows[:, 0] % 64 == 0).all() and fx.term_w.max() == 63
    for nq in tor.MANY_NQS:
        lay = tor.many_layout(nq)
        parts = hybrid_model(fx, lay, True, k, what=(fx.name, nq, k))
        assert [c for _, c, _, _ in parts] == ([1] if nq == 1 else [32, 1])
        for c0, c, g, res in parts:
            assert g["n_slices"] >= 17 and g["n_slices"] * g["slice_rows"] >= fx.n
            # every slice but the first takes its rows' D from beyond the first slice_rows floats of a query's scores
            assert (fx.dsc["asc"][g["slice_rows"]:] > 0).all()
            check_many(res, lay[c0:c0 + c], k, 17, (fx.name, nq, k, c0))
            print(tor.describe(f"{fx.name} nq={nq} k={k} chunk at {c0}", res), "slices", res["slices"])


def _ids(D, S, qual, wd, ws, k):
    import hybrid_reference as href

    return href.search(D[None], S[None], qual, wd, ws, k)[0][0]


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.HYBRID_KS)
def test_hybrid_split_fixtures_are_exact_and_separate_the_orderings(k, mode):
    """sensitivity of the split carrier, on the references alone.  Exact: asserted where a fixture is made (hybrid_split_fixture), restated
    here from the stored values.  Separating: for every busy kind — the kinds whose H rises with the pattern; a constant or a falling
    pattern selects the first k rows whatever is dropped — the top-k by the dense term alone (w_dense * D), by the sparse term alone and
    by H with the two weights swapped (where they differ: (1, 1) and (-1, -1) swapped are themselves) each differ from the top-k by H in
    at least half of the k slots, over the fixture's rows and (allow) over its near miss's."""
    least = {}
    for sd in tor.SPARSE_DTYPES:
        for w in tor.HYBRID_WEIGHTS:
            fx = tor.hybrid_split_fixture(sd, sd, k, mode, w)
            wd, ws = w
            for kk in fx.kinds:
                H = np.float32(wd) * fx.dsc[kk] + np.float32(ws) * fx.ssc[kk]
                assert np.array_equal(H, fx.scores[kk]) and np.array_equal(H.astype(np.float64), fx.intended[kk]), (fx.name, kk)
                for a in (fx.dsc[kk], fx.ssc[kk]):
                    assert np.array_equal(a.astype(np.float16).astype(np.float32), a), (fx.name, kk)
            if sd != "f32":
                continue                                             # (the same D, S and H: asserted above)
            zero = np.zeros(fx.n, np.float32)
            for qual in [fx.permitted()] + ([fx.ok1] if mode == "allow" else []):
                for kk in fx.busy:
                    by_h = _ids(fx.dsc[kk], fx.ssc[kk], qual, wd, ws, k)
                    others = {"dense term alone": _ids(fx.dsc[kk], zero, qual, wd, ws, k), "sparse term alone": _ids(zero, fx.ssc[kk], qual, wd, ws, k)}
                    if wd != ws:
                        others["weights swapped"] = _ids(fx.dsc[kk], fx.ssc[kk], qual, ws, wd, k)
                    for name, ids in others.items():
                        differ = int((ids != by_h).sum())
                        least[name] = min(least.get(name, k), differ)
                        assert 2 * differ >= k, (fx.name, kk, name, differ, k)
    print(f"split k={k} {mode}: the fewest of {k} slots that differ from the top-k by H: {least}")


def test_wrong_hybrid_models_disagree():
    """sensitivity, on the model and the references alone: no kernel is made wrong for this.
    A queue that sorts one entry late (walk's slack = 1) can differ from the right one only where a step ends with count == room + 1 —
    the near-miss kinds, "over" and the ascending rows under ok1 —, and loses the last row of the whole step behind it, the best so far:
    on the fixture's rows up to that step it disagrees with the order rule for every k (further rows overtake the lost one, so the whole
    fixture shows it only where the loss is among the last k rows that push).
    A reader of the dense scores that takes a slice-local row, or the query's index in the call where the chunk's is meant, returns
    another result on the many-slices and on the chunked case."""
    import hybrid_reference as href

    whole = []
    for k in tor.HYBRID_KS:
        L = tor.sparse_L(k)
        plain, masked = tor.hybrid_split_fixture("f32", "f32", k, "plain", (1.0, 1.0)), tor.hybrid_split_fixture("f32", "f32", k, "allow", (-0.5, -4.0))
        for fx, kind, ok in ((plain, "over", np.ones(plain.n, bool)), (masked, "desc", masked.ok1)):
            assert fx.effective[kind] in ("over", "asc")
            H = fx.scores[kind][None]
            cut = None
            for end in range(tor.SPARSE_STEP, fx.n + tor.SPARSE_STEP, tor.SPARSE_STEP):
                if tor.walk(H[:, :end], np.arange(min(end, fx.n)), ok[:end], k, L, tor.SPARSE_STEP)["near_miss"][0]:
                    cut = min(end, fx.n)
                    break
            assert cut is not None, (fx.name, kind)
            late = tor.walk(H[:, :cut], np.arange(cut), ok[:cut], k, L, tor.SPARSE_STEP, slack=1)
            want = tor.reference_topk(H[:, :cut], ok[:cut], k)
            assert not np.array_equal(np.where(late["ids"] == tor.SENT, -1, late["ids"]), want[0]), (fx.name, kind, cut)
            assert late["ids"][0, 0] != want[0][0, 0], (fx.name, kind, "the best row so far is the one lost")
            late = tor.walk(H, np.arange(fx.n), ok, k, L, tor.SPARSE_STEP, slack=1)
            if not np.array_equal(np.where(late["ids"] == tor.SENT, -1, late["ids"]), tor.reference_topk(H, ok, k)[0]):
                whole.append((k, fx.effective[kind]))
    print(f"sorts only above room + 1: disagrees on the whole fixture at {whole}")
    assert {k for k, kind in whole if kind == "over"} >= {127, 128, 255, 256}

    def differs(a, b):
        return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))

    # a slice-local row index: row r of slice s reads the dense score of row r - s * slice_rows
    fx = tor.many_hybrid_fixture()
    for k in tor.MANY_KS:
        for nq in tor.MANY_NQS:
            lay = tor.many_layout(nq)
            for c0, c in tor.hybrid_chunks(fx.n, nq, 0, libbert.test_hybrid_chunk)[0]:
                g = libbert.test_sparse_scan_geometry(0, tor.SPARSE_V, fx.n, c, k)
                local = np.arange(fx.n) % g["slice_rows"]
                for kind in set(lay[c0:c0 + c]) - {"const"}:
                    wrong = href.search(fx.dsc[kind][None, local], fx.ssc[kind][None], np.ones(fx.n, bool), 1.0, 1.0, k)
                    assert differs(wrong, tor.hybrid_reference(fx, k)[kind]), (k, nq, kind)
    # the query's index in the call: chunk c0 .. c0 + c writes rows 0 .. c of the matrix, and query c0 + q reads row c0 + q — beyond the
    # first chunk a row that no chunk of this call has written (zeros here)
    k, nq, pref = tor.HYBRID_CHUNK_K, tor.HYBRID_CHUNK_NQ, tor.HYBRID_CHUNK
    for mode in ("plain", "allow"):
        for w in tor.HYBRID_WEIGHTS:
            fx = tor.hybrid_split_fixture("f32", "f32", k, mode, w)
            lay = tor.layouts(fx.kinds, fx.busy, fx.idle, nq, 2)["mixed"]
            D, S = np.stack([fx.dsc[kk] for kk in lay]), np.stack([fx.ssc[kk] for kk in lay])
            matrix = np.zeros((nq, fx.n), np.float32)
            read = np.zeros_like(D)
            for c0, c in tor.hybrid_chunks(fx.n, nq, pref, libbert.test_hybrid_chunk)[0]:
                matrix[:c] = D[c0:c0 + c]
                read[c0:c0 + c] = matrix[c0:c0 + c]
            assert np.array_equal(read[:pref], D[:pref]) and not np.array_equal(read, D)
            wrong = href.search(read, S, fx.permitted(), *w, k)
            assert differs(wrong, tor.of_layout(tor.hybrid_reference(fx, k), lay)), (fx.name, "call index")
            unchunked = href.search(D, S, fx.permitted(), *w, k)
            assert not differs(unchunked, tor.of_layout(tor.hybrid_reference(fx, k), lay))
