"""Removed rows, allow-lists and compaction of the embedding index (bert_hip_index_remove / _search_filtered / _compact; the masked
instantiations of search.hip's index_topk_kernel).  The yardstick is the unfiltered search: index A holds all rows, index B
only the rows that qualify, in their order; a masked or post-removal search on A must return what the plain search on B
returns, B's ids mapped back through the (monotone) map — the same ids and the same score bits, the -1 / -inf tail included.
That holds exactly: a score depends on its (query, row) pair and dpad alone, and a monotone id map keeps the tie rule."""
import ctypes as C
import os

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = os.path.join(ROOT, "tests", "golden", "sample_client_texts_600.txt")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


class _Hip:
    """Just enough of the HIP runtime through ctypes (the runtime libbert.so itself is linked against)."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        assert self.lib.hipMemcpy(C.c_void_p(p), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0
        return p

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def stream(self):
        s = C.c_void_p()
        assert self.lib.hipStreamCreate(C.byref(s)) == 0
        return s.value

    def free(self, *ps):
        for p in ps:
            self.lib.hipFree(C.c_void_p(p))

    def free_bytes(self):
        free, total = C.c_size_t(), C.c_size_t()
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value


# ---- the yardstick

def plain_on_qualifying(model, dtype, rows, keep, queries, k):
    """the plain search on an index of rows[keep] alone, its ids mapped back to rows' ids"""
    qual = np.nonzero(keep)[0].astype(np.int32)
    b = model.index(dim=rows.shape[1], dtype=dtype)
    if len(qual):
        b.add(rows[qual])
    ids, sc = b.search(queries, k)
    b.close()
    if len(qual) == 0:
        assert (ids == -1).all()
        return ids, sc
    return np.where(ids >= 0, qual[np.maximum(ids, 0)], -1).astype(np.int32), sc


def assert_same(got, want, what):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[0]][:8], wi[bad[0]][:8], gs[bad[0]][:8], ws[bad[0]][:8])


def masks(rng, N):
    """(name, bool [N]) per mask of the issue's list"""
    def m(f):
        a = np.zeros(N, bool)
        f(a)
        return a

    out = [("all ones", np.ones(N, bool)),
           ("all zeros", np.zeros(N, bool)),
           ("one bit", m(lambda a: a.__setitem__(int(rng.integers(N)), True))),
           ("alternating", m(lambda a: a.__setitem__(slice(0, None, 2), True))),
           ("random 0.5", rng.random(N) < 0.5),
           ("random 0.01", rng.random(N) < 0.01),
           ("whole words zero", m(lambda a: (a.__setitem__(slice(None), True), a.__setitem__(slice(128, 1152), False)))),
           ("only the last partial word", m(lambda a: a.__setitem__(slice((N - 1) // 32 * 32, None), True)))]
    if N == 4500:
        # two slices of 2304 rows (max(2048, 16 k) rows at least per slice, rounded up to the 128-row step)
        out.append(("first slice cleared", m(lambda a: a.__setitem__(slice(2304, None), True))))
    return out


def _combos():
    # (dim, N, Q, k), pruned like test_gpu_search.py's grid: every value of every axis appears with every row type; N = 65537 once
    per_dtype = {
        "f32": [(7, 1, 1, 1), (384, 31, 33, 10), (7, 33, 1, 256), (384, 127, 1, 10), (7, 129, 33, 1), (384, 1000, 33, 256),
                (7, 4500, 1, 10), (384, 4500, 33, 1)],
        "f16": [(384, 1, 33, 10), (7, 31, 1, 256), (384, 33, 33, 1), (7, 127, 33, 10), (384, 129, 1, 256), (7, 1000, 1, 1),
                (384, 4500, 33, 10), (384, 65537, 33, 10)],
        "i8": [(7, 1, 33, 256), (384, 31, 1, 1), (7, 33, 33, 10), (384, 127, 33, 256), (7, 129, 1, 10), (384, 1000, 1, 10),
               (384, 4500, 1, 1), (7, 4500, 33, 256)],
    }
    for dtype, cases in per_dtype.items():
        for dim, N, Q, k in cases:
            yield dtype, dim, N, Q, k


@pytest.mark.parametrize("dtype,dim,N,Q,k", list(_combos()))
def test_filter_and_removal_grid(model, dtype, dim, N, Q, k):
    rng = np.random.default_rng(dim * 1000003 + N * 7 + Q * 3 + k)
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    a = model.index(dim=dim, dtype=dtype)
    a.add(rows)
    for name, keep in masks(rng, N):
        want = plain_on_qualifying(model, dtype, rows, keep, queries, k)
        assert_same(a.search(queries, k, allow=keep), want, ("allow", name))
        # the same mask through remove, on an index of its own
        r = model.index(dim=dim, dtype=dtype)
        r.add(rows)
        gone = np.nonzero(~keep)[0]
        assert r.remove(gone) == len(gone)
        assert len(r) == N and r.n_live == int(keep.sum())
        assert_same(r.search(queries, k), want, ("remove", name))
        r.close()
    assert a.n_live == N
    a.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_removal_and_allow_list_intersect(model, dtype):
    rng = np.random.default_rng(77)
    N, dim, Q, k = 4500, 40, 33, 10
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    live, allow = rng.random(N) < 0.6, rng.random(N) < 0.3
    live[256:512] = False                       # words only the removal clears,
    allow[1024:1280] = False                    # words only the allow-list clears
    a = model.index(dim=dim, dtype=dtype)
    a.add(rows)
    a.remove(np.nonzero(~live)[0])
    assert_same(a.search(queries, k, allow=allow), plain_on_qualifying(model, dtype, rows, live & allow, queries, k), "both")
    # uint32 words pass through the binding
    assert_same(a.search(queries, k, allow=pybert.allow_words(allow, N)), a.search(queries, k, allow=allow), "words")
    a.close()


# ---- int8 against the NumPy restatement of its arithmetic (the helpers of test_gpu_search_i8.py, restated)

def quantize(x):
    x = np.asarray(x, dtype=np.float32)
    finite = np.isfinite(x).all(axis=1)
    amax = np.abs(np.where(np.isfinite(x), x, np.float32(0))).max(axis=1, initial=np.float32(0)).astype(np.float32)
    scale = np.where(finite, amax / np.float32(127), np.float32(np.nan)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint(x / scale[:, None])
    keep = (finite & (scale != 0))[:, None]
    return np.where(keep, np.clip(np.where(keep, q, 0), -127, 127), 0).astype(np.int8), scale


def i8_scores(queries, rows):
    qc, qs = quantize(queries)
    rc, rs = quantize(rows)
    dot = qc.astype(np.float64) @ rc.astype(np.float64).T
    with np.errstate(invalid="ignore", over="ignore"):
        return (dot.astype(np.int64).astype(np.float32) * qs[:, None]) * rs[None, :]


def ref_topk(S, k):
    Q, N = S.shape
    ids = np.full((Q, k), -1, np.int32)
    sc = np.full((Q, k), -np.inf, np.float32)
    for i in range(Q):
        s = S[i]
        valid = np.nonzero(~np.isnan(s))[0]
        n = min(k, len(valid))
        if n == 0:
            continue
        v = s[valid]
        kth = np.partition(v, len(v) - n)[len(v) - n]
        cand = valid[v >= kth]
        order = np.lexsort((cand, -s[cand]))[:n]
        ids[i, :n] = cand[order]
        sc[i, :n] = s[cand[order]]
    return ids, sc


def test_i8_filtered_against_the_numpy_restatement(model):
    rng = np.random.default_rng(31)
    N, dim, Q, k = 4500, 200, 33, 10
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    keep = rng.random(N) < 0.5
    keep[128:1152] = False
    S = i8_scores(queries, rows)
    S[:, ~keep] = np.nan                                   # (a NaN score is never returned)
    ix = model.index(dim=dim, dtype="i8")
    ix.add(rows)
    assert_same(ix.search(queries, k, allow=keep), ref_topk(S, k), "i8 allow")
    ix.remove(np.nonzero(~keep)[0])
    assert_same(ix.search(queries, k), ref_topk(S, k), "i8 remove")
    ix.close()


# ---- remove's own rules

@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_remove_rules_and_rows_added_afterwards(model, dtype, capfd):
    rng = np.random.default_rng(3)
    N, dim, k = 300, 24, 10
    rows, more, queries = unit_rows(rng, N, dim), unit_rows(rng, 50, dim), unit_rows(rng, 5, dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    assert ix.remove([]) == 0 and ix.n_live == N
    assert ix.remove([5, 7, 5, 299, 7]) == 3                # repeats count once
    assert ix.remove([5, 6]) == 1                           # an already-removed id is ignored
    assert (len(ix), ix.n_live) == (N, N - 4)
    before = ix.search(queries, k)
    for bad in ([N], [-1], [0, N]):                         # out of [0, size): an error, and nothing changes — row 0 stays
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            ix.remove(bad)
        assert "bert_hip_index_remove" in capfd.readouterr().err
    assert (len(ix), ix.n_live) == (N, N - 4)
    assert_same(ix.search(queries, k), before, "after refused removals")
    keep = np.ones(N + 50, bool)
    keep[[5, 6, 7, 299]] = False
    assert_same(before, plain_on_qualifying(model, dtype, rows, keep[:N], queries, k), "removed")
    # rows added after a removal are live, and their ids go on from size
    assert ix.add(more) == N
    assert (len(ix), ix.n_live) == (N + 50, N + 46)
    every = np.concatenate([rows, more])
    assert_same(ix.search(queries, k), plain_on_qualifying(model, dtype, every, keep, queries, k), "added after removal")
    ids, _ = ix.search(more[:5], 1)
    assert ids[:, 0].tolist() == list(range(N, N + 5))
    # and can be removed in turn
    assert ix.remove([N + 1]) == 1
    keep[N + 1] = False
    assert_same(ix.search(queries, k), plain_on_qualifying(model, dtype, every, keep, queries, k), "a new row removed")
    ix.close()


# ---- the bitmap's own edges at the smallest sizes that have them: the ends of a word, the first capacity step, stray allow bits

@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_removals_at_the_ends_of_a_word_in_seventy_rows(model, dtype):
    rng = np.random.default_rng(70)
    N, dim, k = 70, 32, 8
    rows = unit_rows(rng, N, dim)
    gone = [0, 31, 32, N - 1]
    queries = rows[[0, 32, N - 1]]                          # each asks for a row that is about to go
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    assert ix.search(queries, 1)[0][:, 0].tolist() == [0, 32, N - 1]
    assert ix.remove(gone) == 4 and (len(ix), ix.n_live) == (N, N - 4)
    keep = np.ones(N, bool)
    keep[gone] = False
    got = ix.search(queries, k)
    assert not np.isin(got[0], gone).any() and (got[0] >= 0).all()
    assert_same(got, plain_on_qualifying(model, dtype, rows, keep, queries, k), "the ends of a word")
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_rows_added_across_the_first_capacity_after_removals(model, dtype):
    rng = np.random.default_rng(71)
    N, n_new, dim, k = 1000, 100, 32, 8                     # 1000 rows fit the first capacity (1024), 1100 do not: the rows and the
    rows, new = unit_rows(rng, N, dim), unit_rows(rng, n_new, dim)      # bitmap move to a new allocation
    gone = [0, 31, N - 1]
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    assert ix.remove(gone) == 3
    assert ix.add(new) == N and (len(ix), ix.n_live) == (N + n_new, N + n_new - 3)
    every = np.concatenate([rows, new])
    keep = np.ones(N + n_new, bool)
    keep[gone] = False
    queries = every[[0, N, N + n_new - 1]]                  # a removed row, the first and the last new one
    got = ix.search(queries, k)
    assert not np.isin(got[0], gone).any() and got[0][1:, 0].tolist() == [N, N + n_new - 1]
    assert_same(got, plain_on_qualifying(model, dtype, every, keep, queries, k), "across the first capacity")
    # the rows in front of the move are still removable, the ones behind it too
    assert ix.remove([1, N + 1, 0]) == 2
    keep[[1, N + 1]] = False
    assert_same(ix.search(queries, k), plain_on_qualifying(model, dtype, every, keep, queries, k), "removed after the move")
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_allow_bits_beyond_the_last_row_are_ignored(model, dtype):
    rng = np.random.default_rng(72)
    N, dim, k = 70, 32, 8
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, 3, dim)
    keep = rng.random(N) < 0.5
    keep[N - 1] = True
    words = pybert.allow_words(keep, N).copy()
    assert len(words) == 3
    stray = words.copy()
    stray[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    assert stray[-1] != words[-1]
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    want = plain_on_qualifying(model, dtype, rows, keep, queries, k)
    assert_same(ix.search(queries, k, allow=words), want, "clear")
    assert_same(ix.search(queries, k, allow=stray), want, "stray bits")
    ix.remove([0])                                          # and with the index's own bitmap beside the list
    keep[0] = False
    assert_same(ix.search(queries, k, allow=stray), plain_on_qualifying(model, dtype, rows, keep, queries, k), "stray bits, a removal")
    ix.close()


def test_short_allow_list_is_an_error_and_leaves_the_outputs(model, capfd):
    rng = np.random.default_rng(4)
    N, dim, k = 100, 16, 3
    ix = model.index(dim=dim, dtype="f16")
    ix.add(unit_rows(rng, N, dim))
    q = unit_rows(rng, 2, dim)
    ids = np.full((2, k), 12345, np.int32)
    sc = np.full((2, k), 0.5, np.float32)
    words = np.full(4, 0xFFFFFFFF, np.uint32)               # 100 rows need 4 words
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    args = (q.ctypes.data_as(f32p), k, words.ctypes.data)
    outs = (ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
    capfd.readouterr()
    assert ix.lib.bert_hip_index_search_filtered(ix.ix, 2, *args, 3, *outs) < 0
    assert "bert_hip_index_search_filtered" in capfd.readouterr().err
    assert (ids == 12345).all() and (sc == 0.5).all()
    with pytest.raises(RuntimeError):
        ix.search(q, k, allow=words[:3])
    assert ix.lib.bert_hip_index_search_filtered(ix.ix, 2, *args, 4, *outs) == 0
    assert_same((ids, sc), ix.search(q, k), "four words")
    ix.close()


# ---- paths that must not change

@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_no_removals_null_and_full_allow_give_the_plain_search(model, dtype):
    rng = np.random.default_rng(8)
    N, dim, Q, k = 4500, 72, 33, 10
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(unit_rows(rng, N, dim))
    q = unit_rows(rng, Q, dim)
    want = ix.search(q, k)
    ids = np.empty((Q, k), np.int32)
    sc = np.empty((Q, k), np.float32)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert ix.lib.bert_hip_index_search_filtered(ix.ix, Q, q.ctypes.data_as(f32p), k, None, 0, ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p)) == 0
    assert_same((ids, sc), want, "allow == NULL")
    assert_same(ix.search(q, k, allow=np.ones(N, bool)), want, "all ones")
    assert ix.n_live == N
    ix.close()


# ---- the device entry points

@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_device_entry_after_reserve(model, dtype):
    rng = np.random.default_rng(12)
    N, dim, Q, k, n_new = 4500, 64, 33, 10, 70
    rows, new, q = unit_rows(rng, N, dim), unit_rows(rng, n_new, dim), unit_rows(rng, Q, dim)
    hip = _Hip()
    s = hip.stream()
    ix = model.index(dim=dim, dtype=dtype)
    ix.reserve(N + n_new, max(Q, n_new), k)
    ix.add(rows)
    live, allow = rng.random(N) < 0.7, rng.random(N + n_new) < 0.5
    ix.remove(np.nonzero(~live)[0])
    want = ix.search(q, k, allow=allow[:N])
    words = pybert.allow_words(allow, N + n_new)
    d_q, d_w, d_new = hip.upload(q), hip.upload(words), hip.upload(new)
    d_i, d_s = hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
    before = hip.free_bytes()
    ix.search_device(Q, d_q, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words))
    assert hip.free_bytes() == before                       # within reserve's bounds: no allocation
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), want, "device entry")
    # add_device behind a removal, then a search, on one stream with no host synchronisation in between
    before = hip.free_bytes()
    assert ix.add_device(n_new, d_new, s) == N
    ix.search_device(Q, d_q, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words))
    ix.search_device(n_new, d_new, 1, d_i, d_s, s)          # (every new row finds itself: Q * k >= n_new results fit)
    got_self = hip.download(d_i, (n_new, 1), np.int32)
    assert hip.free_bytes() == before
    assert got_self[:, 0].tolist() == list(range(N, N + n_new))
    ix.search_device(Q, d_q, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words))
    keep = np.concatenate([live, np.ones(n_new, bool)]) & allow
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))),
                plain_on_qualifying(model, dtype, np.concatenate([rows, new]), keep, q, k), "after add_device")
    assert (len(ix), ix.n_live) == (N + n_new, int(live.sum()) + n_new)
    hip.free(d_q, d_w, d_new, d_i, d_s)
    ix.close()


# ---- compaction

@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_compaction(model, dtype):
    rng = np.random.default_rng(15)
    N, dim, Q, k = 4500, 56, 33, 10
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    # without removals: a no-op that returns size
    old = ix.compact()
    assert old.tolist() == list(range(N)) and len(ix) == N
    live = rng.random(N) < 0.4
    live[128:1152] = False
    ix.remove(np.nonzero(~live)[0])
    n_live = ix.n_live
    assert n_live == int(live.sum())
    pre_i, pre_s = ix.search(q, k)
    old = ix.compact()
    assert old.tolist() == np.nonzero(live)[0].tolist()
    assert len(ix) == n_live == ix.n_live
    post_i, post_s = ix.search(q, k)
    assert_same((np.where(post_i >= 0, old[np.maximum(post_i, 0)], -1).astype(np.int32), post_s), (pre_i, pre_s), "compacted")
    # the next row gets id n_live, and a second compaction has nothing to do
    extra = unit_rows(rng, 3, dim)
    assert ix.add(extra) == n_live
    ids, _ = ix.search(extra, 1)
    assert ids[:, 0].tolist() == [n_live, n_live + 1, n_live + 2]
    assert len(ix.compact()) == n_live + 3
    # everything removed, then compacted: an empty, usable index
    ix.remove(np.arange(len(ix)))
    assert len(ix.compact()) == 0 and len(ix) == 0
    ids, sc = ix.search(q, k)
    assert (ids == -1).all() and np.isneginf(sc).all()
    assert ix.add(extra) == 0
    ix.close()


# ---- the text route

def test_search_texts_never_returns_a_removed_row(model):
    with open(TEXTS, encoding="utf-8") as f:
        texts = [line.rstrip("\n") for line in f]
    ix = model.index()
    assert ix.add_texts(texts) == 0
    queries = [texts[7], texts[123], "Should I get health insurance?"]
    pre_i, pre_s = ix.search_texts(queries, 40)
    gone = sorted(set(pre_i[:, :5].ravel().tolist()))       # every query loses its five best
    assert ix.remove(gone) == len(gone) and ix.n_live == len(texts) - len(gone)
    ids, sc = ix.search_texts(queries, 20)
    assert not np.isin(ids, gone).any() and (ids >= 0).all()
    # what is left of the earlier, longer answer, in its order and with its bits
    for q in range(len(queries)):
        left = ~np.isin(pre_i[q], gone)
        assert ids[q].tolist() == pre_i[q][left][:20].tolist()
        assert sc[q].view(np.int32).tolist() == pre_s[q][left][:20].view(np.int32).tolist()
    ix.close()
