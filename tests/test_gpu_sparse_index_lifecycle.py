"""GPU tests of the sparse index's life cycle (bert_hip.h "Sparse index: removing rows, filtered search, rescoring, compaction,
files"): removed rows and allow-lists under the masked scan, rescoring of per-query candidates, compaction, the file form, stream
capture and bert-search --sparse --save / --load.  The reference of every filtered or rescored result is
tests/sparse_index_reference.py: scores(), the rows that do not qualify set to NaN, then topk() — which never returns a NaN.  Equality
means bits, in ids and in scores."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import hip_graph
import sparse_index_file as sf
import sparse_index_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
OK = hip_graph.HIP_SUCCESS
DTYPES = ["f32", "f16"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """(ids, scores or weights) pairs: equal ids, equal bits"""
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _p(a):
    return a.ctypes.data


@pytest.fixture(scope="module")
def model(make_model):
    """any model: a sparse index only needs the context's device"""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


def _terms(rng, n, kk, V, fill, ties):
    """n entries of kk columns: per entry up to fill distinct ids of [0, V), drawn towards 0 so that entries share ids, at random places,
    -1 elsewhere; entry 0 has as many as fit.  ties: weights 1 or 2 (many equal scores, exact in f16), else of both signs over six orders
    of magnitude."""
    ids = np.full((n, kk), -1, np.int32)
    if ties:
        w = rng.integers(1, 3, (n, kk)).astype(np.float32)
    else:
        w = (rng.standard_normal((n, kk)) * 10.0 ** rng.integers(-3, 4, (n, kk))).astype(np.float32)
    top = min(fill, kk, V)
    for r in range(n):
        c = top if r == 0 else int(rng.integers(0, top + 1))
        draw = np.unique((V * rng.random(4 * c + 8) ** 3).astype(np.int64))
        c = min(c, len(draw))
        ids[r, rng.permutation(kk)[:c]] = rng.permutation(draw)[:c]
    return ids, w


def _patterns(n, seed=0):
    """the allow / removal patterns of the issue over n rows, name -> bool [n] (True = the row qualifies)"""
    rng = np.random.default_rng(1000 + n + seed)
    r, nb = np.arange(n), -(-n // 64)
    p = {"all ones": np.ones(n, bool), "all zeros": np.zeros(n, bool)}
    one = np.zeros(n, bool)
    one[np.minimum(64 * np.arange(nb) + (7 * np.arange(nb) + 5) % 64, n - 1)] = True
    p["one bit per block"] = one
    if n >= 192:
        cleared = np.ones(n, bool)
        cleared[64:128] = False
        p["a block cleared between two full ones"] = cleared
    p["only the last block"] = r >= 64 * (nb - 1)
    p["alternating"] = r % 2 == 0
    p["random 50 %"] = rng.random(n) < 0.5
    p["random 1 %"] = rng.random(n) < 0.01
    return p


def _want(sc, qual, k):
    """the reference's top-k over the qualifying rows: the others' scores NaN, which topk never returns"""
    s = np.array(sc, np.float32, copy=True)
    s[:, ~qual] = np.nan
    res = [ref.topk(row, k) for row in s]
    return np.stack([x[0] for x in res]), np.stack([x[1] for x in res])


@dataclasses.dataclass
class Case:
    n: int
    width: int
    V: int
    ties: bool
    nq: int = 3
    kq: int = 16


CASES = {
    "n 1": Case(1, 4, 64, True),
    "n 65, width 256, V 30522": Case(65, 256, 30522, False, kq=64),
    "n 300, width 4, V 64: ties": Case(300, 4, 64, True),
    "n 300, width 256, V 30522": Case(300, 256, 30522, False, kq=64),
    "n 4200, 512 queries: two slices": Case(4200, 4, 64, True, nq=512),
}
_DATA = {}


def _data(name, dtype):
    """rows, stored rows, queries and the reference's scores [nq][n] of a case, computed once"""
    if (name, dtype) not in _DATA:
        c = CASES[name]
        rng = np.random.default_rng(len(name) + c.n)
        ids, w = _terms(rng, c.n, c.width, c.V, c.width, c.ties)
        q_ids, q_w = _terms(rng, c.nq, c.kq, c.V, c.kq, c.ties)
        if c.n == 1:
            # query 1 asks for the single row's terms: a score that is not +0
            used = ids[0][ids[0] >= 0]
            q_ids[1], q_w[1] = -1, 1.0
            q_ids[1, :len(used)] = used
        st = ref.stored_rows(ids, w, c.width, dtype)
        sc = ref.scores(st[0], st[1], q_ids, q_w, c.V)
        assert c.n > 1 or sc[1, 0] > 0
        for a in (ids, w, q_ids, q_w, sc, *st):
            a.setflags(write=False)
        _DATA[(name, dtype)] = (ids, w, st, q_ids, q_w, sc)
    return _DATA[(name, dtype)]


def _index(model, name, dtype):
    c = CASES[name]
    ids, w = _data(name, dtype)[:2]
    ix = model.sparse_index(c.width, dtype, n_vocab=c.V)
    assert ix.add(ids, w) == 0
    return ix


def _poisoned_words(mask):
    """the mask's words with every bit at and beyond len(mask) set and three words of ones behind them"""
    n = len(mask)
    words = pybert.allow_words(mask, n).copy()
    if n % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    return np.concatenate([words, np.full(3, 0xFFFFFFFF, np.uint32)])


# ------------------------------------------------------------------------------------------------
# 1. filtered search
# ------------------------------------------------------------------------------------------------
SMALL = [n for n in CASES if CASES[n].nq == 3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SMALL)
def test_allow_lists_and_removals_equal_the_reference(model, name, dtype):
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    if c.ties and c.n > 1:
        assert max(len(np.unique(s)) for s in sc) < c.n // 4               # many equal scores: the order rule decides
    ix = _index(model, name, dtype)
    plain = ix.search(q_ids, q_w, 10)
    pats = _patterns(c.n)
    names = list(pats)
    for pi, pname in enumerate(names):
        qual = pats[pname]
        for k in (10, 256):
            want = _want(sc, qual, k)
            if qual.sum() < k:
                assert (want[0][:, qual.sum():] == -1).all() and np.isneginf(want[1][:, qual.sum():]).all()
            assert _same(ix.search(q_ids, q_w, k, allow=qual), want), (pname, k)
            # words beyond ceil(size / 32) and bits at and beyond size are the caller's: all ones here
            assert _same(ix.search(q_ids, q_w, k, allow=_poisoned_words(qual)), want), (pname, k)
        if pname == "all ones":
            assert _same(ix.search(q_ids, q_w, 10, allow=qual), plain)
        # the same pattern as removals, alone and under the next pattern as an allow-list
        rm = _index(model, name, dtype)
        gone = np.flatnonzero(~qual).astype(np.int32)
        assert rm.remove(gone) == len(gone) and rm.n_live == qual.sum() and len(rm) == c.n
        assert _same(rm.search(q_ids, q_w, 10), _want(sc, qual, 10)), pname
        assert _same(rm.search(q_ids[:1], q_w[:1], 256), _want(sc[:1], qual, 256)), pname
        other = pats[names[(pi + 3) % len(names)]]
        assert _same(rm.search(q_ids, q_w, 10, allow=_poisoned_words(other)), _want(sc, qual & other, 10)), pname
        rm.close()
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_slices_under_a_mask(model, dtype):
    name = "n 4200, 512 queries: two slices"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    g = pybert.test_sparse_scan_geometry(DTYPES.index(dtype), c.V, c.n, c.nq, 10)
    assert g["n_slices"] == 2 and c.n % g["slice_rows"] != 0, g
    ix = _index(model, name, dtype)
    pats = _patterns(c.n)
    qual = pats["random 50 %"]
    assert _same(ix.search(q_ids, q_w, 10, allow=qual), _want(sc, qual, 10))
    # removals over both slices — the whole second slice but one row — and an allow-list on top
    keep = pats["a block cleared between two full ones"].copy()
    keep[g["slice_rows"]:-1] = False
    assert ix.remove(np.flatnonzero(~keep)) == (~keep).sum()
    assert _same(ix.search(q_ids, q_w, 10), _want(sc, keep, 10))
    assert _same(ix.search(q_ids[:5], q_w[:5], 10, allow=pats["alternating"]), _want(sc[:5], keep & pats["alternating"], 10))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_allow_list_of_exactly_the_words_needed(model, hip, dtype):
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    ix = _index(model, name, dtype)
    qual = _patterns(c.n)["random 50 %"]
    words = pybert.allow_words(qual, c.n)
    assert len(words) == 10                                                 # ceil(300 / 32): nothing behind them belongs to the caller
    d_allow, d_qi, d_qw = hip.upload(words), hip.upload(q_ids), hip.upload(q_w)
    d_ids, d_sc = hip.nans((c.nq, 10), np.int32), hip.nans((c.nq, 10))
    ix.search_device(c.nq, c.kq, d_qi, d_qw, 10, d_ids, d_sc, 0, d_allow, len(words))
    assert _same((hip.download(d_ids, (c.nq, 10), np.int32), hip.download(d_sc, (c.nq, 10))), _want(sc, qual, 10))
    # too few words are refused
    with pytest.raises(ValueError):
        ix.search_device(c.nq, c.kq, d_qi, d_qw, 10, d_ids, d_sc, 0, d_allow, 9)
    with pytest.raises(ValueError):
        ix.search(q_ids, q_w, 10, allow=words[:9])
    hip.free(d_allow, d_qi, d_qw, d_ids, d_sc)
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clear_lanes_terms_never_enter_a_score(model, dtype):
    """the disallowed rows are full (count = width, large weights on every id the queries ask for), the allowed ones hold one term: a
    block is walked to the largest count of its QUALIFYING rows, and what the others hold reaches no score"""
    rng = np.random.default_rng(3)
    V, width, n = 64, 32, 200
    ids = np.full((n, width), -1, np.int32)
    w = np.zeros((n, width), np.float32)
    qual = rng.random(n) < 0.3
    qual[64:128] = False                                                    # a block without a qualifying row
    for r in range(n):
        if qual[r]:
            ids[r, 0], w[r, 0] = rng.integers(0, V), rng.integers(1, 4)
        else:
            ids[r], w[r] = rng.permutation(V)[:width], 1000.0
    q_ids = np.stack([rng.permutation(V)[:32] for _ in range(3)]).astype(np.int32)
    q_w = rng.integers(1, 5, (3, 32)).astype(np.float32)
    st = ref.stored_rows(ids, w, width, dtype)
    sc = ref.scores(st[0], st[1], q_ids, q_w, V)
    assert sc[:, ~qual].min() >= 1000.0 and sc[:, qual].max() < 100.0
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    for k in (10, 256):
        assert _same(ix.search(q_ids, q_w, k, allow=qual), _want(sc, qual, k))
    ix.remove(np.flatnonzero(~qual))
    assert _same(ix.search(q_ids, q_w, 256), _want(sc, qual, 256))
    ix.close()


# ------------------------------------------------------------------------------------------------
# 2. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_filtered_result_depends_on_its_query_and_the_qualifying_rows_alone(model, hip, dtype):
    name = "n 4200, 512 queries: two slices"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    ix = _index(model, name, dtype)
    qual = _patterns(c.n)["random 50 %"]
    probe = (q_ids[5:6], q_w[5:6])
    alone = ix.search(*probe, 100, allow=qual)
    assert _same(alone, _want(sc[5:6], qual, 100))
    for pos in range(7):
        b_ids, b_w = q_ids[10:17].copy(), q_w[10:17].copy()
        b_ids[pos], b_w[pos] = probe[0][0], probe[1][0]
        got = ix.search(b_ids, b_w, 100, allow=qual)
        assert _same((got[0][pos:pos + 1], got[1][pos:pos + 1]), alone), pos
    top10 = ix.search(*probe, 10, allow=qual)
    assert _same(top10, (alone[0][:, :10], alone[1][:, :10]))
    words = pybert.allow_words(qual, c.n)
    d_allow, d_qi, d_qw = hip.upload(words), hip.upload(probe[0]), hip.upload(probe[1])
    d_ids, d_sc = hip.nans((1, 100), np.int32), hip.nans((1, 100))
    ix.search_device(1, c.kq, d_qi, d_qw, 100, d_ids, d_sc, 0, d_allow, len(words))
    assert _same((hip.download(d_ids, (1, 100), np.int32), hip.download(d_sc, (1, 100))), alone)
    hip.free(d_allow, d_qi, d_qw, d_ids, d_sc)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 3. rescore
# ------------------------------------------------------------------------------------------------
def _rescore_want(sc_row, cand, live, k):
    """one query: every entry of cand that names a live row of [0, n) counts, as often as it appears; larger score first, equal
    scores smaller id first"""
    ent = [(float(sc_row[i]), int(i)) for i in cand if 0 <= i < len(sc_row) and live[i]]
    ent.sort(key=lambda e: (-e[0], e[1]))
    out_i, out_s = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32)
    for j, (_, i) in enumerate(ent[:k]):
        out_i[j], out_s[j] = i, sc_row[i]
    return out_i, out_s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_cand", [1, 64, 65, 1024])
def test_rescore_is_the_filtered_search_over_the_candidates(model, n_cand, dtype):
    name = "n 4200, 512 queries: two slices"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    nq = 3
    q_ids, q_w, sc = q_ids[:nq], q_w[:nq], sc[:nq]
    rng = np.random.default_rng(n_cand)
    ix = _index(model, name, dtype)
    removed = rng.permutation(c.n)[:c.n // 3].astype(np.int32)
    ix.remove(removed)
    live = np.ones(c.n, bool)
    live[removed] = False
    # distinct ids per query, removed ones among them, a fifth of the places -1
    cand = np.stack([rng.permutation(c.n)[:n_cand] for _ in range(nq)]).astype(np.int32)
    cand[rng.random(cand.shape) < 0.2] = -1
    if n_cand >= 64:
        assert (~live[cand[cand >= 0]]).any() and (cand == -1).any()
    for k in sorted({1, min(10, n_cand), 256}):                           # k < n_cand, k > n_cand
        got = ix.rescore(q_ids, q_w, cand, k)
        for q in range(nq):
            allow = np.zeros(c.n, bool)
            allow[cand[q][cand[q] >= 0]] = True
            want = ix.search(q_ids[q:q + 1], q_w[q:q + 1], k, allow=allow)
            assert _same((got[0][q:q + 1], got[1][q:q + 1]), want), (k, q)
            assert _same(want, _want(sc[q:q + 1], allow & live, k))
    # a repeated id counts as often as it appears
    if n_cand >= 64:
        rep = cand.copy()
        rep[:, 1::2] = rep[:, 0:-1:2]
        got = ix.rescore(q_ids, q_w, rep, 256)
        for q in range(nq):
            want = _rescore_want(sc[q], rep[q], live, 256)
            assert _same((got[0][q], got[1][q]), want), q
        valid = [int(i) for i in rep[0] if i >= 0 and live[i]]
        assert len(valid) > len(set(valid))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rescore_device_counts_bad_ids_as_none_and_stays_in_bounds(model, hip, dtype):
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    rng = np.random.default_rng(9)
    nq, n_cand, k, G = 3, 65, 80, 256
    ix = _index(model, name, dtype)
    ix.remove(np.arange(0, c.n, 3))
    live = np.ones(c.n, bool)
    live[::3] = False
    cand = np.stack([rng.permutation(c.n)[:n_cand] for _ in range(nq)]).astype(np.int32)
    flat = cand.reshape(-1)
    for j, bad in zip(rng.permutation(flat.size)[:30], np.resize([c.n, c.n + 1, -2, -7, 2 ** 31 - 1, -2 ** 31, 1 << 20, -1], 30)):
        flat[j] = bad
    want = [_rescore_want(sc[q], cand[q], live, k) for q in range(nq)]
    want = np.stack([x[0] for x in want]), np.stack([x[1] for x in want])
    assert (want[0] == -1).any()                                            # k exceeds the valid candidates

    def guarded(payload, dtype_):
        """a device buffer [G canaries | payload | G canaries]; returns (base, pointer to the payload, check)"""
        canary = np.full(G, 0x5A5A5A5A, np.uint32).view(dtype_)
        host = np.concatenate([canary, payload.reshape(-1), canary])
        base = hip.upload(host)

        def check(payload_unchanged):
            now = hip.download(base, host.shape, dtype_)
            assert np.array_equal(now[:G].view(np.uint32), canary.view(np.uint32)) and np.array_equal(now[-G:].view(np.uint32), canary.view(np.uint32))
            if payload_unchanged:
                assert np.array_equal(now.view(np.uint32), host.view(np.uint32))
            return now[G:-G]
        return base, base + 4 * G, check

    b_c, p_c, c_c = guarded(cand, np.int32)
    b_qi, p_qi, c_qi = guarded(np.array(q_ids[:nq]), np.int32)
    b_qw, p_qw, c_qw = guarded(np.array(q_w[:nq]), np.float32)
    b_oi, p_oi, c_oi = guarded(np.full((nq, k), -9, np.int32), np.int32)
    b_os, p_os, c_os = guarded(np.full((nq, k), np.nan, np.float32), np.float32)
    ix.rescore_device(nq, c.kq, p_qi, p_qw, n_cand, p_c, k, p_oi, p_os)
    hip.sync()
    for chk in (c_c, c_qi, c_qw):
        chk(True)
    assert _same((c_oi(False).reshape(nq, k), c_os(False).reshape(nq, k)), want)
    # the host form refuses what the device form skips, outputs untouched
    out_i, out_s = np.full((nq, k), 7, np.int32), np.full((nq, k), 7.0, np.float32)
    q_i, q_x = np.array(q_ids[:nq]), np.array(q_w[:nq])
    assert model.lib.bert_hip_sparse_index_rescore(ix.ix, nq, c.kq, _p(q_i), _p(q_x), n_cand, _p(cand), k, _p(out_i), _p(out_s)) == -2
    assert (out_i == 7).all() and (out_s == 7.0).all()
    ok = np.where((cand >= -1) & (cand < c.n), cand, -1).astype(np.int32)
    assert _same(ix.rescore(q_i, q_x, ok, k), want)
    hip.free(b_c, b_qi, b_qw, b_oi, b_os)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 4. remove, add, compact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_add_compact(model, hip, dtype):
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    ix = model.sparse_index(c.width, dtype, n_vocab=c.V)
    ix.add(ids[:70], w[:70])
    assert ix.n_live == 70 and np.array_equal(ix.live_ids(), np.arange(70))
    assert ix.remove([3, 3, 69, 40]) == 3 and ix.remove([40, 5]) == 1 and ix.remove([]) == 0
    live = np.ones(c.n, bool)
    live[[3, 69, 40, 5]] = False
    assert ix.n_live == 66 and len(ix) == 70
    assert _same(ix.get_rows([3, 69]), (st[0][[3, 69]], st[1][[3, 69]]))     # get_rows still returns removed rows
    # rows added after a removal are live: 70 .. 89 starts and ends inside word 2; then on the device, across a block edge
    assert ix.add(ids[70:90], w[70:90]) == 70
    assert _same(ix.search(q_ids, q_w, 256), _want(sc[:, :90], live[:90], 256))
    d_i, d_w = hip.upload(ids[90:300]), hip.upload(w[90:300])
    assert ix.add_device(210, c.width, d_i, d_w) == 90
    hip.sync()
    hip.free(d_i, d_w)
    assert len(ix) == 300 and ix.n_live == 296
    assert _same(ix.search(q_ids, q_w, 256), _want(sc, live, 256))
    assert np.array_equal(ix.live_ids(), np.flatnonzero(live))
    ix.remove(np.arange(100, 200))
    live[100:200] = False
    before = ix.search(q_ids, q_w, 256)
    assert _same(before, _want(sc, live, 256))
    # compact: the live rows in their order, their stored bits, the same search through old_ids
    old = ix.compact()
    assert np.array_equal(old, np.flatnonzero(live)) and len(ix) == ix.n_live == live.sum()
    assert _same(ix.get_rows(np.arange(len(old))), (st[0][old], st[1][old]))
    after = ix.search(q_ids, q_w, 256)
    mapped = np.where(after[0] >= 0, old[np.maximum(after[0], 0)], -1)
    assert _same((mapped, after[1]), before)
    assert _same(after, ix.search(q_ids, q_w, 256, allow=np.ones(len(old), bool)))
    again = ix.compact()
    assert np.array_equal(again, np.arange(len(old))) and len(ix) == len(old)            # a no-op
    # the compacted index goes on: add, remove everything, compact to nothing, add again
    assert ix.add(ids[:5], w[:5]) == len(old) and ix.n_live == len(old) + 5
    ix.remove(np.arange(len(ix)))
    assert ix.n_live == 0 and (ix.search(q_ids, q_w, 4)[0] == -1).all()
    assert len(ix.compact()) == 0 and len(ix) == 0
    assert ix.add(ids[:65], w[:65]) == 0
    assert _same(ix.search(q_ids, q_w, 10), _want(sc[:, :65], np.ones(65, bool), 10))
    ix.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_index_and_outputs_untouched(model, dtype, capfd):
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    L = model.lib
    ix = _index(model, name, dtype)
    ix.remove([7])
    q_i, q_x = np.array(q_ids), np.array(q_w)
    out_i, out_s = np.full((3, 4), 7, np.int32), np.full((3, 4), 7.0, np.float32)
    words = np.full(10, 0xFFFFFFFF, np.uint32)
    cand = np.zeros((3, 4), np.int32)
    capfd.readouterr()

    def refused(r, what):
        err = capfd.readouterr().err
        assert r == -2 and what in err, (r, what, err)
        assert len(ix) == 300 and ix.n_live == 299 and (out_i == 7).all() and (out_s == 7.0).all()

    for bad in (-1, 300):
        refused(L.bert_hip_sparse_index_remove(ix.ix, 2, _p(np.array([8, bad], np.int32))), "outside")
    refused(L.bert_hip_sparse_index_remove(ix.ix, 2, None), "pointer")
    refused(L.bert_hip_sparse_index_remove(ix.ix, -1, _p(cand)), "n >= 0")
    refused(L.bert_hip_sparse_index_search_filtered(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, _p(words), 9, _p(out_i), _p(out_s)), "allow-list")
    refused(L.bert_hip_sparse_index_search_filtered_device(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, _p(words), 9, _p(out_i), _p(out_s), None), "allow-list")
    refused(L.bert_hip_sparse_index_search_filtered(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 0, _p(words), 10, _p(out_i), _p(out_s)), "k must be")
    refused(L.bert_hip_sparse_index_search_filtered(ix.ix, 3, c.kq, None, _p(q_x), 4, _p(words), 10, _p(out_i), _p(out_s)), "pointers")
    for n_cand in (0, 1025):
        refused(L.bert_hip_sparse_index_rescore(ix.ix, 3, c.kq, _p(q_i), _p(q_x), n_cand, _p(cand), 4, _p(out_i), _p(out_s)), "n_cand")
        refused(L.bert_hip_sparse_index_rescore_device(ix.ix, 3, c.kq, None, None, n_cand, None, 4, None, None, None), "n_cand")
    for k in (0, 257):
        refused(L.bert_hip_sparse_index_rescore(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, _p(cand), k, _p(out_i), _p(out_s)), "k must be")
    refused(L.bert_hip_sparse_index_rescore(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, None, 4, _p(out_i), _p(out_s)), "pointers")
    for bad in (-2, 300):
        cb = cand.copy()
        cb[2, 3] = bad
        refused(L.bert_hip_sparse_index_rescore(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, _p(cb), 4, _p(out_i), _p(out_s)), "candidate")
    bad_q = q_i.copy()
    bad_q[1, 0] = c.V
    refused(L.bert_hip_sparse_index_rescore(ix.ix, 3, c.kq, _p(bad_q), _p(q_x), 4, _p(cand), 4, _p(out_i), _p(out_s)), "outside")
    refused(L.bert_hip_sparse_index_save(ix.ix, None), "path")
    refused(L.bert_hip_sparse_index_save(ix.ix, b""), "path")
    # n_queries == 0 is a no-op; allow == NULL is the plain search and ignores n_words
    assert L.bert_hip_sparse_index_rescore(ix.ix, 0, c.kq, None, None, 4, None, 4, None, None) == 0
    assert L.bert_hip_sparse_index_search_filtered(ix.ix, 3, c.kq, _p(q_i), _p(q_x), 4, None, 0, _p(out_i), _p(out_s)) == 0
    live = np.ones(c.n, bool)
    live[7] = False
    assert _same((out_i, out_s), _want(sc, live, 4))
    ix.close()


# ------------------------------------------------------------------------------------------------
# 5. save and load
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_save_load_round_trip(model, tmp_path, n, dtype):
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    for removals in (False, True):
        ix = model.sparse_index(c.width, dtype, n_vocab=c.V)
        if n:
            ix.add(ids[:n], w[:n])
        live = np.ones(n, bool)
        if removals and n:
            live[::3] = False
            ix.remove(np.flatnonzero(~live))
        path = str(tmp_path / f"{n}_{int(removals)}.spx")
        ix.save(path)
        assert not os.path.exists(path + ".tmp") and os.path.getsize(path) == sf.file_bytes(DTYPES.index(dtype), c.width, n, int(removals and n > 0))
        back = model.load_sparse_index(path)
        assert (back.width, back.dtype, back.n_vocab) == (c.width, dtype, c.V)            # n_vocab is the file's, not the model's
        assert len(back) == n and back.n_live == live.sum()
        for x in (ix, back):
            for k in (10, 256):
                assert _same(x.search(q_ids, q_w, k), _want(sc[:, :n], live, k)), (removals, k)
        if n:
            assert _same(back.get_rows(np.arange(n)), (st[0][:n], st[1][:n]))
            allow = np.arange(n) % 2 == 0
            assert _same(back.search(q_ids, q_w, 10, allow=allow), _want(sc[:, :n], live & allow, 10))
            # a loaded index goes on like any other
            assert back.add(ids[:3], w[:3]) == n and back.remove([n]) == 1 and back.n_live == live.sum() + 2
        ix.close()
        back.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_files_bytes_depend_on_rows_and_removals_alone(model, tmp_path, dtype):
    name = "n 300, width 256, V 30522"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    a, b = model.sparse_index(c.width, dtype, n_vocab=c.V), model.sparse_index(c.width, dtype, n_vocab=c.V)
    a.reserve(5000, 4, 10)
    a.add(ids, w)
    for lo, hi in ((0, 1), (1, 63), (63, 130), (130, 300)):                   # grown, in parts that start and end inside blocks
        b.add(ids[lo:hi], w[lo:hi])
    files = []
    for x, removed in ((a, [5, 299, 64]), (b, [64, 5, 299, 5])):
        p0, p1 = str(tmp_path / f"{len(files)}_plain.spx"), str(tmp_path / f"{len(files)}_removed.spx")
        x.save(p0)
        x.remove(removed)
        x.save(p1)
        files.append((open(p0, "rb").read(), open(p1, "rb").read()))
    assert files[0][0] == files[1][0] and files[0][1] == files[1][1]
    assert len(files[0][1]) == len(files[0][0]) + 40                        # the live words of 300 rows
    # the file reads back as documented
    f = sf.parse(files[0][1])
    assert (f["version"], f["dtype"], f["n_vocab"], f["width"], f["n_rows"], f["has_live"]) == (1, DTYPES.index(dtype), c.V, c.width, 300, 1)
    assert f["ids"].shape == (5, c.width, 64)
    assert np.array_equal(f["counts"], (st[0] >= 0).sum(1))
    assert _same(sf.rows_of(f), st)
    live = np.ones(300, bool)
    live[[5, 299, 64]] = False
    assert np.array_equal(f["live"], pybert.allow_words(live, 300))
    # zeros behind every count and in the rows of the last block at and beyond n_rows
    flat_i = f["ids"].transpose(0, 2, 1).reshape(-1, c.width)
    flat_w = f["weights"].transpose(0, 2, 1).reshape(-1, c.width)
    assert not flat_i[300:].any() and not flat_w[300:].view(np.uint16 if dtype == "f16" else np.uint32).any()
    behind = np.arange(c.width)[None, :] >= f["counts"][:, None]
    assert not flat_i[:300][behind].any() and not flat_w[:300][behind].view(np.uint16 if dtype == "f16" else np.uint32).any()
    assert sf.parse(files[0][0])["live"] is None
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# 5b. the bitmap's own edges at the smallest sizes that have them: the ends of a word, the first capacity step, a file written twice
# ------------------------------------------------------------------------------------------------
_EDGE = {}
_MARKED = [0, 31, 32, 69, 999, 1000, 1099]


def _edge_data(dtype):
    """1100 rows of width 8 over 512 ids and three queries, with the reference's scores, computed once.  The rows _MARKED hold the one
    term (511, 20000 + 32 j) — exact in f16 — and query 0 asks for id 511 alone: its answer is the marked rows, the last first."""
    if dtype not in _EDGE:
        rng = np.random.default_rng(812)
        ids, w = _terms(rng, 1100, 8, 512, 8, False)
        q_ids, q_w = _terms(rng, 3, 8, 512, 8, False)
        for j, r in enumerate(_MARKED):
            ids[r], w[r] = -1, 1.0
            ids[r, 0], w[r, 0] = 511, 20000.0 + 32 * j
        q_ids[0], q_w[0] = -1, 1.0
        q_ids[0, 0] = 511
        st = ref.stored_rows(ids, w, 8, dtype)
        sc = ref.scores(st[0], st[1], q_ids, q_w, 512)
        for a in (ids, w, q_ids, q_w, sc):
            a.setflags(write=False)
        _EDGE[dtype] = (ids, w, q_ids, q_w, sc)
    return _EDGE[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_removals_at_the_ends_of_a_word_in_seventy_rows(model, tmp_path, dtype):
    ids, w, q_ids, q_w, sc = _edge_data(dtype)
    n, k, gone = 70, 8, [0, 31, 32, 69]
    ix = model.sparse_index(8, dtype, n_vocab=512)
    assert ix.add(ids[:n], w[:n]) == 0
    assert ix.search(q_ids, q_w, k)[0][0, :4].tolist() == [69, 32, 31, 0]          # what is about to go is what query 0 finds
    assert ix.remove(gone) == 4 and len(ix) == n and ix.n_live == n - 4
    live = np.ones(n, bool)
    live[gone] = False
    got = ix.search(q_ids, q_w, k)
    assert not np.isin(got[0], gone).any()
    assert _same(got, _want(sc[:, :n], live, k))
    # remove -> save -> load: size, live rows and answers are the saved index's, and a second save gives the first one's bytes
    p1, p2 = str(tmp_path / "a.spx"), str(tmp_path / "b.spx")
    ix.save(p1)
    back = model.load_sparse_index(p1)
    assert len(back) == n and back.n_live == n - 4
    assert _same(back.search(q_ids, q_w, k), got)
    back.save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    ix.close()
    back.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_added_across_the_first_capacity_after_removals(model, dtype):
    ids, w, q_ids, q_w, sc = _edge_data(dtype)
    n, n_new, k, gone = 1000, 100, 8, [0, 31, 999]          # 1000 rows fit the first capacity (1024), 1100 do not: the blocks and the
    ix = model.sparse_index(8, dtype, n_vocab=512)          # bitmap move to a new allocation
    assert ix.add(ids[:n], w[:n]) == 0 and ix.remove(gone) == 3
    assert ix.add(ids[n:], w[n:]) == n and len(ix) == n + n_new and ix.n_live == n + n_new - 3
    live = np.ones(n + n_new, bool)
    live[gone] = False
    got = ix.search(q_ids, q_w, k)
    assert got[0][0, :4].tolist() == [1099, 1000, 69, 32]                           # the new rows are found, the removed ones are not
    assert not np.isin(got[0], gone).any()
    assert _same(got, _want(sc, live, k))
    # rows in front of the move and behind it are removable afterwards
    assert ix.remove([1000, 32, 0]) == 2
    live[[1000, 32]] = False
    assert _same(ix.search(q_ids, q_w, k), _want(sc, live, k))
    ix.close()


def _damaged(data, dtype_code, width, n):
    """(name, bytes) of every damaged form of a good file of n rows with live words"""
    arr = sf.array_bytes(dtype_code, width, n)
    eb = 2 if dtype_code == 1 else 4
    def patched(off, b):
        d = bytearray(data)
        d[off:off + len(b)] = b
        return bytes(d)
    def field(i, v):
        return patched(8 + 4 * i, struct.pack("<I", v))
    counts = np.frombuffer(data, "<i4", n, 64 + 2 * arr)
    row = int(np.flatnonzero(counts > 0)[-1])                              # a row with a used column
    id_off = 64 + ((row // 64 * width + int(counts[row]) - 1) * 64 + row % 64) * eb
    yield "truncated by one byte", data[:-1]
    yield "one byte long", data[:1]
    yield "wrong magic", b"BHIPIDX1" + data[8:]
    yield "version 2", field(0, 2)
    yield "dtype 2", field(1, 2)
    yield "width 0", field(3, 0)
    yield "width 257", field(3, 257)
    yield "n_vocab 0", field(2, 0)
    if dtype_code == 1:
        yield "dtype 1 with n_vocab 65537", field(2, 65537)
    yield "a reserved byte set", patched(40, b"\1")
    yield "has_live 2", field(5, 2)
    yield "a count of width + 1", patched(64 + 2 * arr + 4 * 3, struct.pack("<i", width + 1))
    yield "a used id = n_vocab", patched(id_off, int(64).to_bytes(eb, "little"))
    yield "a live bit set beyond n_rows", data[:-1] + bytes([data[-1] | 0x80])


_DAMAGE_NAMES = ["truncated by one byte", "one byte long", "wrong magic", "version 2", "dtype 2", "width 0", "width 257", "n_vocab 0",
                 "dtype 1 with n_vocab 65537", "a reserved byte set", "has_live 2", "a count of width + 1", "a used id = n_vocab",
                 "a live bit set beyond n_rows"]


@pytest.fixture(scope="module")
def good_files(model, tmp_path_factory):
    """a saved index of 65 rows with removals, per dtype: (path, bytes)"""
    name = "n 300, width 4, V 64: ties"
    c = CASES[name]
    out = {}
    for dtype in DTYPES:
        ids, w = _data(name, dtype)[:2]
        ix = model.sparse_index(c.width, dtype, n_vocab=c.V)
        ix.add(ids[:65], w[:65])
        ix.remove([1])
        path = str(tmp_path_factory.mktemp("spx") / f"good_{dtype}.spx")
        ix.save(path)
        ix.close()
        out[dtype] = (path, open(path, "rb").read())
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("damage", _DAMAGE_NAMES)
def test_damaged_files_are_refused(model, good_files, tmp_path, capfd, damage, dtype):
    path, data = good_files[dtype]
    cases = dict(_damaged(data, DTYPES.index(dtype), 4, 65))
    if damage not in cases:
        assert dtype == "f32" and damage == "dtype 1 with n_vocab 65537"
        # (an f32 file: dtype 1 and n_vocab 65537 written together)
        cases[damage] = data[:12] + struct.pack("<II", 1, 65537) + data[20:]
    bad = tmp_path / "bad.spx"
    bad.write_bytes(cases[damage])
    capfd.readouterr()
    assert not model.lib.bert_hip_sparse_index_load(model.ctx, os.fsencode(str(bad)))
    err = capfd.readouterr().err
    assert "bert_hip_sparse_index_load" in err and "bad.spx" in err, err
    with pytest.raises(RuntimeError):
        model.load_sparse_index(str(bad))
    # the good file still loads
    back = model.load_sparse_index(path)
    assert len(back) == 65 and back.n_live == 64
    back.close()


def test_load_refuses_a_missing_file(model, tmp_path, capfd):
    capfd.readouterr()
    assert not model.lib.bert_hip_sparse_index_load(model.ctx, os.fsencode(str(tmp_path / "none.spx")))
    assert "cannot read" in capfd.readouterr().err
    assert not model.lib.bert_hip_sparse_index_load(model.ctx, None)
    assert "no path" in capfd.readouterr().err


# ------------------------------------------------------------------------------------------------
# 6. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_device_after_removals_and_filtered_search_in_one_capture(model, hip, dtype):
    name = "n 4200, 512 queries: two slices"
    c = CASES[name]
    ids, w, st, q_ids, q_w, sc = _data(name, dtype)
    nq, k, n0, n1 = 9, 10, 3000, 3070
    q_i, q_x = np.array(q_ids[:nq]), np.array(q_w[:nq])
    gone = np.arange(5, n0, 7)
    qual = _patterns(n1)["random 50 %"]
    words = pybert.allow_words(qual, n1)
    eager = model.sparse_index(c.width, dtype, n_vocab=c.V)
    eager.add(ids[:n0], w[:n0])
    eager.remove(gone)
    eager.add(ids[n0:n1], w[n0:n1])
    want = eager.search(q_i, q_x, k, allow=qual)
    live = np.ones(n1, bool)
    live[gone] = False
    assert _same(want, _want(sc[:nq, :n1], live & qual, k))
    ix = model.sparse_index(c.width, dtype, n_vocab=c.V)
    ix.reserve(n1, nq, k)
    ix.add(ids[:n0], w[:n0])
    ix.remove(gone)                                                         # (the bitmap is sized with the reserved rows)
    d = [hip.upload(a) for a in (np.array(ids[n0:n1]), np.array(w[n0:n1]), q_i, q_x, words)]
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    s = hip.stream()
    first = []
    with hip.capture(s) as cap:
        first.append(model.lib.bert_hip_sparse_index_add_device(ix.ix, n1 - n0, c.width, d[0], d[1], s))
        first.append(model.lib.bert_hip_sparse_index_search_filtered_device(ix.ix, nq, c.kq, d[2], d[3], k, d[4], len(words), d_ids, d_sc, s))
    assert first == [n0, 0] and cap.status == OK and cap.graph and len(ix) == n1 and ix.n_live == n1 - len(gone)
    assert (hip.download(d_ids, (nq, k), np.int32) == -1).all(), "capturing must run nothing"
    assert hip.kernel_nodes(cap.graph) == 5                      # add, live bits, query images, masked scan, merge
    ex = hip.instantiate(cap.graph)
    for launch in range(2):
        hip.poison(d_ids, (nq, k), np.int32)
        hip.poison(d_sc, (nq, k))
        hip.launch(ex, s)
        assert _same((hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k))), want), launch
    assert _same(ix.search(q_i, q_x, k, allow=qual), want)
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(*d, d_ids, d_sc)
    ix.close()
    eager.close()


# ------------------------------------------------------------------------------------------------
# 7. bert-search --sparse --save / --load
# ------------------------------------------------------------------------------------------------
def test_bert_search_sparse_save_then_load_prints_the_same(model_dir, tok_golden, tmp_path):
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    path = os.path.join(model_dir, "sparse_index_lifecycle_text.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=True), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    rng = np.random.default_rng(8)
    lines = [" ".join(rng.choice(words, size=int(m), replace=False)) for m in rng.integers(3, 12, size=10)]
    file = tmp_path / "lines.txt"
    file.write_text("\n".join(lines) + "\n")
    saved = tmp_path / "lines.spx"
    exe = os.path.join(BIN, "bert-search")
    queries = "\n".join(lines[:4]) + "\nq\n"
    built = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "32", "-k", "5", "--save", str(saved)], input=queries,
                           capture_output=True, text=True, timeout=300)
    assert built.returncode == 0 and saved.exists() and not (tmp_path / "lines.spx.tmp").exists(), built.stderr
    assert built.stdout.count("Closest texts:") == 4 and "similarity score" in built.stdout
    loaded = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "32", "-k", "5", "--load", str(saved)], input=queries,
                            capture_output=True, text=True, timeout=300)
    assert loaded.returncode == 0 and loaded.stdout == built.stdout, loaded.stderr
    # another number of lines than the file's rows, and the dense-only options, are refused
    file.write_text("\n".join(lines[:9]) + "\n")
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "--load", str(saved)], input="q\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "holds 10 rows" in r.stderr
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "--i8"], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sparse goes with" in r.stderr
