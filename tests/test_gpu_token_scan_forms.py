"""Every instantiation of token_index_scan_kernel (token_index.hip) on ordered and exact-fit scores: f16 plain and masked, int8 plain,
masked and listed (the int8 rescore).  test_gpu_token_index_order.py drives the f16 plain one to its list's edges; here the other four
meet the same edges through fixtures of their own (topk_order_reference.py: "int8 token fixtures", "masked token fixtures", "listed
fixtures"), whose states test_topk_order_host.py proves on the CPU.  Two host paths of the int8 form run here for the first time:
TokenIndex::scan_chunks past one chunk of queries, whose query workspace is quantised again per chunk, and the quantisation of more
rows than one launch takes (QUANT_MAX_ROWS = 2^22).

Nothing here has a tolerance: ids and score bits must equal the order rule over the expected matrix — the closed form of the f16
fixtures, token_i8_reference.scores_i8 of the int8 ones — and the host model of the kernel's walk, compared with
token_index_reference.same_result."""
import numpy as np
import pytest

import token_i8_reference as t8
import token_index_reference as tref
import topk_order_reference as tor
from bert_cpp_amd import pybert
from hip_graph import Hip

from test_gpu_late_i8 import _as_f16, _device_rescore, _device_search

pytestmark = pytest.mark.gpu

CHUNK = 256                              # TokenIndex::QCHUNK (token_index.h)
QUANT_MAX_ROWS = 1 << 22                 # rows per launch of token_i8_quantize_kernel (token_index.hip)
SCANS = ["token_index_scan", "token_index_scan_masked", "token_i8_scan", "token_i8_scan_masked", "token_i8_rescore"]


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    m.profile(True)
    yield m
    m.set_option("token_index_slices", "0")
    m.close()


def _index(model, form, rows, cu, dim=tor.TOKEN_DIM):
    ix = model.token_index(dim, form)
    assert ix.add(rows, cu) == 0 and len(ix) == len(cu) - 1 and ix.n_tokens() == int(cu[-1] - cu[0])
    return ix


_LAUNCHES = {name: 0 for name in SCANS + ["token_i8_quantize", "topk_merge"]}
_WALKS = {}


def _launches(model):
    """the launches of the module's model so far, by the profiler's label (a report clears the profiler's counts: they are added up
    here)"""
    for name, stat in model.profile_report().items():
        if name in _LAUNCHES:
            _LAUNCHES[name] += stat["launches"]
    return dict(_LAUNCHES)


def _rows_of(got, want, labels):
    """the queries whose row of got is not want's"""
    return [lab for i, lab in enumerate(labels) if not tref.same_result((got[0][i:i + 1], got[1][i:i + 1]), (want[0][i:i + 1], want[1][i:i + 1]))]


def _search_both(model, hip, ix, q, qcu, max_q_len, k, slices, allow=None):
    """(search, search_device) under the tuning key `slices`; allow: a bool array, given to the device form as words"""
    model.set_option("token_index_slices", str(slices))
    try:
        words = None if allow is None else pybert.allow_words(allow, len(ix))
        return ix.search(q, qcu, k, allow=allow), _device_search(hip, ix, q, qcu, max_q_len, k, words)
    finally:
        model.set_option("token_index_slices", "0")


def _check_search(model, hip, ix, fx, kinds, lens, q, qcu, k, slices, ok, allow, what):
    """search and search_device of the kinds against the order rule over the documents ok and against the model of the walk that the
    cut `slices` gives"""
    S = np.stack([fx.scores[kk] for kk in kinds])
    want = tor.reference_topk(S, ok, k)
    n_slices, slice_docs = pybert.test_token_index_plan(fx.n, len(kinds), slices)
    key = (fx.name, tuple(kinds), k, n_slices, slice_docs, np.broadcast_to(ok, fx.n).tobytes())
    if key not in _WALKS:                                            # (the modes of one mask walk alike)
        res = tor.token_search(S, k, n_slices, slice_docs, ok)
        _WALKS[key] = res["ids"], res["scores"]
    walked = _WALKS[key]
    assert tref.same_result(walked, want), (what, "the model")
    labels = list(zip(kinds, lens))
    for name, res in zip(("search", "search_device"), _search_both(model, hip, ix, q, qcu, max(lens), k, slices, allow)):
        assert _rows_of(res, want, labels) == [], (what, name)
        assert tref.same_result(res, walked), (what, name)


# ------------------------------------------------------------------------------------------------
# 1. int8, plain
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_int8_search_on_ordered_and_exact_fit_sequences(model, k):
    """one index per pattern — ascending, sawtooth, the staircase of this k, its near miss —, every kind (+e_0, -e_0, zero) at query
    lengths 1 and 33: as one slice (25 steps, the last of 37 documents) and as planned (slices of 17 documents)"""
    hip = Hip()
    for pattern in tor.TOKEN_I8_PATTERNS:
        fx = tor.token_i8_fixture(pattern, k)
        kinds, lens = tor.token_i8_layout(fx)
        q, qcu = tor.token_i8_queries(kinds, lens)
        ix = _index(model, "i8", fx.rows, fx.cu)
        for slices in (1, 0):
            _check_search(model, hip, ix, fx, kinds, lens, q, qcu, k, slices, True, None, (k, pattern, slices))
        ix.close()


def test_int8_search_over_seventeen_slices_and_two_merge_rounds(model):
    k = tor.TOKEN_MANY_K
    fx = tor.token_i8_fixture("asc", n=tor.TOKEN_MANY_DOCS)
    kinds, lens = tor.token_i8_layout(fx)
    q, qcu = tor.token_i8_queries(kinds, lens)
    hip = Hip()
    ix = _index(model, "i8", fx.rows, fx.cu)
    _check_search(model, hip, ix, fx, kinds, lens, q, qcu, k, tor.TOKEN_MANY_SLICES, True, None, "17 slices")
    ix.close()


# ------------------------------------------------------------------------------------------------
# 2. masked, f16 and int8
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tor.TOKEN_KS)
@pytest.mark.parametrize("form", ["f16", "i8"])
def test_masked_search_on_the_exact_fit_and_its_near_miss(model, form, k):
    """fit_mask of this k over the ascending pattern and its near miss, each as an allow-list, as removals and as both: one slice, the
    planned cut and 7 slices (which start inside a mask word); then the index without removals is searched without an allow-list and
    runs the unmasked kernel"""
    fx = tor.token_fixture(k) if form == "f16" else tor.token_i8_fixture("asc")
    kinds = [kk for kk in tor.TOKEN_MASK_KINDS for _ in tor.TOKEN_QUERY_LENS]
    lens = [ln for _ in tor.TOKEN_MASK_KINDS for ln in tor.TOKEN_QUERY_LENS]
    q, qcu = tor.token_queries(kinds, lens) if form == "f16" else tor.token_i8_queries(kinds, lens)
    plain_label, masked_label = ("token_index_scan", "token_index_scan_masked") if form == "f16" else ("token_i8_scan", "token_i8_scan_masked")
    hip = Hip()
    plain = _index(model, form, fx.rows, fx.cu)
    for mask, name in zip(tor.token_masks(k), ("exact fit", "near miss")):
        for mode in tor.TOKEN_MASK_MODES:
            removed, allow = tor.token_mask_mode(mask, mode)
            ix = plain if mode == "allow" else _index(model, form, fx.rows, fx.cu)
            if len(removed):
                assert ix.remove(removed) == len(removed)
            assert ix.n_live() == fx.n - len(removed) and len(ix) == fx.n
            assert ix.n_live_tokens() == int(fx.lens.sum() - fx.lens[removed].sum())
            before = _launches(model)
            for slices in tor.TOKEN_MASK_SLICES:
                _check_search(model, hip, ix, fx, kinds, lens, q, qcu, k, slices, mask, allow, (form, k, name, mode, slices))
            after = _launches(model)
            assert after[masked_label] == before[masked_label] + 2 * len(tor.TOKEN_MASK_SLICES) and after[plain_label] == before[plain_label]
            if ix is not plain:
                ix.close()
    # afterwards, without an allow-list: the unmasked kernel, and every document again
    before = _launches(model)
    _check_search(model, hip, plain, fx, kinds, lens, q, qcu, k, 0, True, None, (form, k, "no allow-list afterwards"))
    after = _launches(model)
    assert after[plain_label] == before[plain_label] + 2 and after[masked_label] == before[masked_label]
    plain.close()


# ------------------------------------------------------------------------------------------------
# 3. listed: the int8 rescore
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_int8_rescore_walks_candidate_positions(model, k):
    """candidate lists that carry their pattern along the positions (tor.candidate_lists): position == id, ids that fall while the scores
    rise, holes of every kind where the masked exact fit pushes nothing, the staircase as repeated ids; as one slice of 1024 positions
    and as planned (64 slices of 16)"""
    fx = tor.listed_fixture()
    kinds, lens = tor.token_i8_layout(fx)
    q, qcu = tor.token_i8_queries(kinds, lens)
    S = np.stack([fx.scores[kk] for kk in kinds])
    labels = list(zip(kinds, lens))
    hip = Hip()
    indexes = {}
    for name, (cand, removed) in tor.candidate_lists(k).items():
        key = removed.tobytes()
        if key not in indexes:
            indexes[key] = _index(model, "i8", fx.rows, fx.cu)
            if len(removed):
                assert indexes[key].remove(removed) == len(removed)
        ix = indexes[key]
        valid = tor.list_valid(cand, removed)
        want = tref.rescore_expected(tor.list_scores(S, cand, removed), np.tile(cand, (len(kinds), 1)), k)
        # the host form refuses ids outside [-1, n_docs): it gets the holes as -1 and as removed ids only
        host = np.where((cand < 0) | (cand >= fx.n), -1, cand)
        assert np.array_equal(tor.list_valid(host, removed), valid)
        for slices in (1, 0):
            n_slices, slice_pos = pybert.test_token_index_plan(len(cand), len(kinds), slices)
            walked = tor.listed_search(S, cand, valid, k, n_slices, slice_pos)
            assert tref.same_result((walked["ids"], walked["scores"]), want), (k, name, slices, "the model")
            model.set_option("token_index_slices", str(slices))
            try:
                got = ix.rescore(q, qcu, np.tile(host, (len(kinds), 1)), k)
                dev = _device_rescore(hip, ix, q, qcu, np.tile(cand, (len(kinds), 1)), k)
            finally:
                model.set_option("token_index_slices", "0")
            for entry, res in (("rescore", got), ("rescore_device", dev)):
                assert _rows_of(res, want, labels) == [], (k, name, slices, entry)
                assert tref.same_result(res, (walked["ids"], walked["scores"])), (k, name, slices, entry)
            if name == "repeats":
                # a repeated id counts each time: under "desc" document 0 (score 0, the best) comes back as often as the list names it
                zeros = int((cand == 0).sum())
                for i, kk in enumerate(kinds):
                    if kk == "desc":
                        assert zeros >= 3 and (dev[0][i][:min(k, zeros)] == 0).all() and (got[0][i][:min(k, zeros)] == 0).all(), (k, slices)
                        assert k <= zeros or dev[0][i][zeros] == 1
    for ix in indexes.values():
        ix.close()


# ------------------------------------------------------------------------------------------------
# 4. int8: more queries than one internal chunk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [CHUNK + 1, 2 * CHUNK + 1])
def test_int8_calls_of_more_queries_than_a_chunk(model, nq):
    """one-token queries that cycle through the kinds: every row of search, search_device, rescore and rescore_device equals the same
    query served in a call of its own, and the order rule"""
    k, n_cand = 10, 33
    fx = tor.token_i8_fixture("asc", n=200)
    kinds = [fx.kinds[i % len(fx.kinds)] for i in range(nq)]
    q, qcu = tor.token_i8_queries(kinds, [1] * nq)
    S = np.stack([fx.scores[kk] for kk in kinds])
    want = tor.reference_topk(S, True, k)
    cand = np.random.default_rng(nq).integers(-1, fx.n, (nq, n_cand)).astype(np.int32)         # -1 entries and repeated ids
    want_r = tref.rescore_expected(S, cand, k)
    hip = Hip()
    ix = _index(model, "i8", fx.rows, fx.cu)
    first = {kk: kinds.index(kk) for kk in fx.kinds}                                            # (the queries of a kind are the same bits)
    alone_kind = {kk: ix.search(q[i:i + 1], [0, 1], k) for kk, i in first.items()}
    alone = np.concatenate([alone_kind[kk][0] for kk in kinds]), np.concatenate([alone_kind[kk][1] for kk in kinds])
    alone_r = [ix.rescore(q[i:i + 1], [0, 1], cand[i:i + 1], k) for i in range(nq)]
    alone_r = np.concatenate([a[0] for a in alone_r]), np.concatenate([a[1] for a in alone_r])
    assert tref.same_result(alone, want) and tref.same_result(alone_r, want_r)
    before = _launches(model)
    for name, got, ref in (("search", ix.search(q, qcu, k), alone), ("search_device", _device_search(hip, ix, q, qcu, 1, k), alone),
                           ("rescore", ix.rescore(q, qcu, cand, k), alone_r), ("rescore_device", _device_rescore(hip, ix, q, qcu, cand, k), alone_r)):
        assert got[0].shape == (nq, k) and _rows_of(got, ref, list(range(nq))) == [], (nq, name)
    after = _launches(model)
    chunks = -(-nq // CHUNK)
    assert after["token_i8_scan"] - before["token_i8_scan"] == 2 * chunks and after["token_i8_rescore"] - before["token_i8_rescore"] == 2 * chunks
    ix.close()


def test_int8_query_workspace_of_a_later_chunk_holds_no_stale_query(model):
    """the int8 form quantises every chunk's queries into the same workspace [QCHUNK][max_q_len], and the quantiser leaves a guarded
    query's slots and the slots behind a query's end alone: in the second chunk they hold the first chunk's bytes.  Query 0 (33 tokens,
    a NaN in token 20) and query 1 (33 good tokens) fill slots 0 and 1; query 256 — the second chunk's slot 0 — is one good token,
    query 257 is empty, query 258 is good"""
    k, L33 = 10, 33
    fx = tor.token_i8_fixture("asc", n=200)
    rng = np.random.default_rng(33)
    long_bad = _as_f16(rng.standard_normal((L33, tor.TOKEN_DIM)))
    long_bad[20, 3] = np.nan
    long_good = rng.standard_normal((L33, tor.TOKEN_DIM))
    long_good[:, 0] = np.abs(long_good[:, 0]) + 1                       # (every token of it scores: none of its slots is a zero)
    long_good = _as_f16(long_good)                                      # (f16 values: the device form is given what the reference scores)
    nq = CHUNK + 4
    one = lambda i: np.array([[(-1.0) ** i * (1 + i % 7), 0, 0, 0, 0, 0, 0, 0]], np.float32)
    parts = [long_bad, long_good] + [one(i) for i in range(2, nq)]
    parts[CHUNK + 1] = np.zeros((0, tor.TOKEN_DIM), np.float32)          # the empty query
    q = np.concatenate(parts)
    qcu = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    assert qcu[1] == 33 and qcu[2] == 66 and qcu[CHUNK + 2] == qcu[CHUNK + 1] and qcu[CHUNK + 1] - qcu[CHUNK] == 1
    good = [i for i in range(nq) if i not in (0, CHUNK + 1)]
    good_rows = np.concatenate([parts[i] for i in good])
    good_cu = np.concatenate([[0], np.cumsum([len(parts[i]) for i in good])]).astype(np.int32)
    S = t8.scores_i8(good_rows, good_cu, fx.rows, fx.cu)
    assert np.isfinite(S).all()
    want = tor.reference_topk(S, True, k)
    hip = Hip()
    ix = _index(model, "i8", fx.rows, fx.cu)
    got = _device_search(hip, ix, q, qcu, L33, k)
    for bad in (0, CHUNK + 1):
        assert (got[0][bad] == -1).all() and np.isneginf(got[1][bad]).all(), bad
    assert _rows_of((got[0][good], got[1][good]), want, good) == []
    # each of the second chunk's queries, and the long one, as it is served alone
    for i in (1, CHUNK, CHUNK + 2, CHUNK + 3):
        alone = _device_search(hip, ix, parts[i], [0, len(parts[i])], L33, k)
        assert tref.same_result((got[0][i:i + 1], got[1][i:i + 1]), alone), i
    # the rescore's workspace is sized for the longest query a search takes; the same queries over every document
    every = np.tile(np.arange(fx.n, dtype=np.int32), (nq, 1))
    resc = _device_rescore(hip, ix, q, qcu, every, k)
    for bad in (0, CHUNK + 1):
        assert (resc[0][bad] == -1).all() and np.isneginf(resc[1][bad]).all(), bad
    assert _rows_of((resc[0][good], resc[1][good]), want, good) == []
    ix.close()


# ------------------------------------------------------------------------------------------------
# 5. the quantisation of more rows than one launch takes
# ------------------------------------------------------------------------------------------------
def test_int8_add_of_more_rows_than_one_quantise_launch(model):
    """2^22 + 37 f16 rows at dim 8 in documents of 4096 tokens: the second launch's offsets into the source rows, the codes and the
    scales.  The rows are a table of 4096 distinct rows tiled; element 7 carries the document's number, so that no two documents hold
    the same rows"""
    dim, per = tor.TOKEN_DIM, 4096
    T = QUANT_MAX_ROWS + 37
    n_docs = -(-T // per)
    table = np.random.default_rng(22).standard_normal((per, dim)).astype(np.float16)
    rows = np.tile(table, (n_docs, 1))[:T]
    rows[:, 7] = ((np.arange(T) // per + 1) / 1024.0).astype(np.float16)
    cu = np.minimum(np.arange(n_docs + 1, dtype=np.int64) * per, T).astype(np.int32)
    assert n_docs == 1025 and cu[-1] == T and cu[-1] - cu[-2] == 37 and cu[1024] == QUANT_MAX_ROWS
    for a, b in ((QUANT_MAX_ROWS - 1, QUANT_MAX_ROWS), (QUANT_MAX_ROWS, QUANT_MAX_ROWS + 1), (0, QUANT_MAX_ROWS)):
        assert not np.array_equal(rows[a], rows[b])
    hip = Hip()
    ix = model.token_index(dim, "i8")
    d_rows = hip.upload(rows)
    assert ix.add_device(cu, d_rows) == 0
    hip.sync()
    hip.free(d_rows)
    assert len(ix) == n_docs and ix.n_tokens() == T
    doc =lambda i: rows[cu[i]:cu[i + 1]].astype(np.float32)
    for i in (0, 1023, 1024):                                            # the first; the last of the first launch; the second launch's, which is the last
        codes, scales = ix.get_codes(i)
        wc, ws = t8.quantise(doc(i))
        assert np.array_equal(codes, wc) and np.array_equal(scales.view(np.uint32), ws.view(np.uint32)), i
    q = np.zeros((1, dim), np.float32)
    q[0, 7] = 1.0                                                        # the later documents score higher: the second launch's is in play
    ids, sc = ix.search(q, [0, 1], 4)
    assert (ids[0] >= 0).all() and len(set(ids[0].tolist())) == 4 and (np.diff(sc[0]) <= 0).all()
    for j, i in enumerate(ids[0].tolist()):
        want = t8.scores_i8(q, [0, 1], doc(i), [0, cu[i + 1] - cu[i]])[0, 0]
        assert np.float32(sc[0][j]).view(np.uint32) == np.float32(want).view(np.uint32) and want != 0, (j, i)
    print(f"top 4 of {n_docs} documents: ids {ids[0].tolist()} scores {sc[0].tolist()}")
    ix.close()


# ------------------------------------------------------------------------------------------------
# 6. masked and listed int8 at the smallest and the largest dim
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [8, 1024])
def test_int8_masked_and_listed_at_other_dims(model, dim):
    """random rows, 130 documents of tref.DOC_LENS, queries of every length: a random 50 % allow-list, a removal set and a rescore of 70
    random candidates with holes, against scores_i8.  dim 1024: the masked and the listed compile with four trips of the k0 loop"""
    import maxsim_reference as mr

    n = 130
    rng = np.random.default_rng(6000 + dim)
    d, dcu = tref.documents(rng, n, dim)
    q, qcu, _ = mr.packed_set(rng, tref.QUERY_LENS, dim)
    d, q = _as_f16(d), _as_f16(q)
    nq = len(qcu) - 1
    S = t8.scores_i8(q, qcu, d, dcu)
    assert S.shape == (nq, n) and np.isfinite(S).all()
    allow = rng.random(n) < 0.5
    gone = np.flatnonzero(rng.random(n) < 0.3).astype(np.int32)
    live = np.ones(n, bool)
    live[gone] = False
    cand = rng.integers(-1, n, (nq, 70)).astype(np.int32)
    wild = cand.copy()
    wild[:, 3], wild[:, 7], wild[:, 11] = n, -7, 2 ** 31 - 1
    hip = Hip()
    plain, removed = _index(model, "i8", d, dcu, dim), _index(model, "i8", d, dcu, dim)
    assert removed.remove(gone) == len(gone) and removed.n_live() == n - len(gone)
    Sm = np.array(S)
    Sm[:, ~live] = np.nan
    before = _launches(model)
    for k in (1, 256):
        for ok, ix, al, what in ((allow, plain, allow, "allow"), (live, removed, None, "removed"), (live & allow, removed, allow, "both")):
            want = tor.reference_topk(S, ok, k)
            for name, res in zip(("search", "search_device"), _search_both(model, hip, ix, q, qcu, 128, k, 0, al)):
                assert tref.same_result(res, want), (dim, k, what, name)
        assert tref.same_result(plain.rescore(q, qcu, cand, k), tref.rescore_expected(S, cand, k)), (dim, k)
        assert tref.same_result(removed.rescore(q, qcu, cand, k), tref.rescore_expected(Sm, cand, k)), (dim, k)
        assert tref.same_result(_device_rescore(hip, removed, q, qcu, wild, k), tref.rescore_expected(Sm, wild, k)), (dim, k)
    after = _launches(model)
    assert after["token_i8_scan_masked"] - before["token_i8_scan_masked"] == 12 and after["token_i8_rescore"] - before["token_i8_rescore"] == 6
    plain.close(); removed.close()


# ------------------------------------------------------------------------------------------------
# 7. which kernels ran
# ------------------------------------------------------------------------------------------------
def test_every_instantiation_was_launched(model):
    """(last in the file; stands alone) one tiny search per instantiation, then the profiler's launch counts"""
    fx = tor.token_i8_fixture("asc", n=200)
    kinds = list(fx.kinds)
    allow = np.arange(fx.n) % 3 != 0
    before = _launches(model)
    q, qcu = tor.token_i8_queries(kinds, [1] * 3)
    # (the f16 form of the same rows: one product by +-1, the values themselves)
    exact = np.stack([np.float32(tor.TOKEN_I8_SIGN[kk]) * tor.values(fx.ranks) + np.float32(0) for kk in kinds])
    for form, S in (("f16", exact), ("i8", np.stack([fx.scores[kk] for kk in kinds]))):
        ix = _index(model, form, fx.rows, fx.cu)
        assert tref.same_result(ix.search(q, qcu, 5), tor.reference_topk(S, True, 5)), form
        assert tref.same_result(ix.search(q, qcu, 5, allow=allow), tor.reference_topk(S, allow, 5)), form
        cand = np.tile(np.arange(40, dtype=np.int32), (3, 1))
        assert tref.same_result(ix.rescore(q, qcu, cand, 5), tref.rescore_expected(S, cand, 5)), form
        ix.close()
    after = _launches(model)
    for name in SCANS + ["token_i8_quantize", "topk_merge"]:
        print(f"{name}: launches {after[name]} (this test: {after[name] - before[name]})")
        assert after[name] > 0 and after[name] > before[name], name
