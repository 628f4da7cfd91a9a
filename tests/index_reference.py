"""NumPy references of the embedding index, shared by test_gpu_index_shapes.py and test_gpu_kmeans_shapes.py.  Nothing here
touches the GPU or the library: the stored forms, the i8 and b1 scores restated bit for bit (as test_gpu_search_i8.py and
test_gpu_search_b1.py state them), the float64 rule of test_gpu_search.py for the f32 and f16 forms restricted to a set of
permitted rows, the row -> list and query -> probed lists rules of the partition, and the data builders whose list lengths are
known by construction.  The ctypes HIP shim is the one of the other index tests."""
import ctypes as C

import numpy as np

DTYPES = ["f32", "f16", "i8", "b1"]
TOL = 2e-6                                                           # per score: TOL * sum_i |q_i r_i| (test_gpu_search.py)
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


class Hip:
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


def unit(x):
    x = np.asarray(x, dtype=np.float32)
    return (x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-30)).astype(np.float32)


def assert_same(got, want, what=""):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[0]][:8], wi[bad[0]][:8], gs[bad[0]][:8], ws[bad[0]][:8])


# ---- the stored forms

def quantize(x):
    """x [n, dim] -> (codes int8 [n, dim], scales float32 [n]): the i8 form's quantizer, in float32"""
    x = np.asarray(x, dtype=np.float32)
    finite = np.isfinite(x).all(axis=1)
    amax = np.abs(np.where(np.isfinite(x), x, np.float32(0))).max(axis=1, initial=np.float32(0)).astype(np.float32)
    scale = np.where(finite, amax / np.float32(127), np.float32(np.nan)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint(x / scale[:, None])
    keep = (finite & (scale != 0))[:, None]
    return np.where(keep, np.clip(np.where(keep, q, 0), -127, 127), 0).astype(np.int8), scale


def restate_rows(rows, dtype):
    """the stored row as bert_hip.h states it (what get_rows returns), in NumPy f32 arithmetic.  The i8 line is the one of
    test_gpu_search_probe.py with the quantizer above, which also takes an all-zero row (scale 0, codes 0) and a non-finite
    one (scale NaN)"""
    rows = np.asarray(rows, dtype=np.float32)
    if dtype == "f32":
        return rows
    if dtype == "f16":
        return rows.astype(np.float16).astype(np.float32)
    if dtype == "b1":
        with np.errstate(invalid="ignore"):
            return np.where(rows > 0, np.float32(1), np.float32(-1))
    codes, scale = quantize(rows)
    with np.errstate(invalid="ignore"):
        return codes.astype(np.float32) * scale[:, None]            # (int8 codes: no -0)


def stored_queries(queries, dtype):
    """the query of a float form as its score reads it"""
    return restate_rows(queries, dtype) if dtype in ("f32", "f16") else np.asarray(queries, dtype=np.float32)


# ---- i8, b1: the scores bit for bit

def exact_scores(queries, rows, dtype):
    """[Q, N] float32: ((float)dot * qscale) * rscale (i8), (float)dot * qscale (b1), over the exact integer dot"""
    qc, qs = quantize(queries)
    if dtype == "i8":
        rc, rs = quantize(rows)
        # codes are at most 127 in size and dim <= 2048: every partial sum is an integer below 2^53, exact in float64
        dot = qc.astype(np.float64) @ rc.astype(np.float64).T
        with np.errstate(invalid="ignore", over="ignore"):
            return (dot.astype(np.int64).astype(np.float32) * qs[:, None]) * rs[None, :]
    assert dtype == "b1"
    with np.errstate(invalid="ignore"):
        bits = np.asarray(rows, dtype=np.float32) > 0
    dot = qc.astype(np.float64) @ np.where(bits, 1.0, -1.0).T
    with np.errstate(invalid="ignore"):
        return dot.astype(np.float32) * qs[:, None]


def ref_topk(S, k):
    """larger score first, equal scores by smaller id, NaN never returned, -1 / -inf beyond"""
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


# ---- f32, f16: float64 on the stored values

class FloatScores:
    """exact [Q, N] float64 scores of the stored values and their tolerances TOL * sum_i |q_i r_i|, computed once per index"""

    def __init__(self, queries, rows, dtype):
        q64 = stored_queries(queries, dtype).astype(np.float64)
        r64 = restate_rows(rows, dtype).astype(np.float64)
        self.exact = q64 @ r64.T
        self.tol = TOL * (np.abs(q64) @ np.abs(r64).T)


def f32_chain_scores(queries, rows):
    """[Q, N] float32: the f32 form's score as bert_hip.h states it, an f32 fma chain, in the order search.hip documents for
    v_mfma_f32_32x32x2_f32 — step (g, e) adds k = 8 g + e, then k = 8 g + 4 + e — with every fma correctly rounded (a
    product of two f32 is exact in float64, and the sum is rounded once to f32 up to a double rounding of 2^-29 ulp).
    Slow, for the CPU checks of the fixtures: what the tolerance of check_float asks of a correct kernel."""
    q = np.asarray(queries, dtype=np.float32).astype(np.float64)
    r = np.asarray(rows, dtype=np.float32).astype(np.float64)
    pad = -q.shape[1] % 8
    q, r = np.pad(q, ((0, 0), (0, pad))), np.pad(r, ((0, 0), (0, pad)))
    acc = np.zeros((len(q), len(r)), np.float32)
    for g in range(q.shape[1] // 8):
        for e in range(4):
            for kk in (8 * g + e, 8 * g + 4 + e):
                acc = (acc.astype(np.float64) + q[:, kk, None] * r[None, :, kk]).astype(np.float32)
    return acc


def check_float(got, fs, permitted, k, what=""):
    """check_results of test_gpu_search.py with the rows of a query restricted to permitted [Q, N] bool: each returned score
    within its tolerance of the exact one; ids permitted, unique, in descending score order; every permitted row whose exact
    score beats the k-th exact score by more than twice its tolerance present, and no returned row more than twice its
    tolerance below it; -1 / -inf beyond the permitted rows"""
    ids, sc = got
    Q, N = fs.exact.shape
    assert ids.shape == (Q, k) and sc.shape == (Q, k) and permitted.shape == (Q, N), what
    for i in range(Q):
        perm = permitted[i] & ~np.isnan(fs.exact[i])
        n_ret = min(k, int(perm.sum()))
        assert (ids[i, n_ret:] == -1).all() and np.isneginf(sc[i, n_ret:]).all(), (what, i, n_ret, ids[i], sc[i])
        g, s = ids[i, :n_ret], sc[i, :n_ret]
        assert ((g >= 0) & (g < N)).all() and len(set(g.tolist())) == n_ret, (what, i, g)
        assert perm[g].all(), (what, i, g[~perm[g]])
        assert (np.diff(s) <= 0).all(), (what, i, s)
        if n_ret == 0:
            continue
        ex, tl = fs.exact[i], fs.tol[i]
        err = np.abs(s.astype(np.float64) - ex[g])
        assert (err <= tl[g] + 1e-30).all(), (what, i, g[err > tl[g] + 1e-30][:5], float((err / (tl[g] + 1e-30)).max()))
        kth = np.sort(ex[perm])[::-1][n_ret - 1]
        must = perm & (ex > kth + 2 * tl)
        assert np.isin(np.nonzero(must)[0], g).all(), (what, i, np.setdiff1d(np.nonzero(must)[0], g)[:5], kth)
        assert (ex[g] >= kth - 2 * tl[g]).all(), (what, i, g[ex[g] < kth - 2 * tl[g]][:5], kth)


def check_against_reference(got, dtype, queries, rows, permitted, k, scores=None, what=""):
    """a result against the reference of its form: bit for bit (i8, b1) or by the float64 rule (f32, f16); scores: what
    scores_of gave for these queries and rows, computed here if None"""
    if scores is None:
        scores = scores_of(queries, rows, dtype)
    if dtype in ("i8", "b1"):
        S = scores.copy()
        S[~permitted] = np.nan                                       # (a NaN score is never returned)
        assert_same(got, ref_topk(S, k), what)
    else:
        check_float(got, scores, permitted, k, what)


def scores_of(queries, rows, dtype):
    """what check_against_reference takes as scores, computed once for many calls: the [Q, N] float32 scores themselves (i8,
    b1) or the FloatScores (f32, f16)"""
    return exact_scores(queries, rows, dtype) if dtype in ("i8", "b1") else FloatScores(queries, rows, dtype)


# ---- the partition

def check_lists(lists, stored, centroids, what=""):
    """row -> list: the list of a row is accepted if its float64 score against the stored row is within the two scores'
    tolerances (at most twice the larger) of the best; if it ties the best exactly, it is the smallest list id that does.
    A stored row that holds a NaN belongs to list 0."""
    x, c = stored.astype(np.float64), centroids.astype(np.float64)
    lists = np.asarray(lists)
    assert lists.shape == (len(x),) and ((lists >= 0) & (lists < len(c))).all(), what
    for r0 in range(0, len(x), 256):
        xs, got = x[r0:r0 + 256], lists[r0:r0 + 256]
        with np.errstate(invalid="ignore"):
            ex = xs @ c.T
            tl = TOL * (np.abs(xs) @ np.abs(c).T)
        nan = np.isnan(ex).any(axis=1)
        assert (got[nan] == 0).all(), (what, r0, np.nonzero(nan)[0][:5])
        ex, tl, got = ex[~nan], tl[~nan], got[~nan]
        ar = np.arange(len(ex))
        best = ex.argmax(axis=1)                                     # (the first of equal maxima: the smallest list id)
        gap = ex[ar, best] - ex[ar, got]
        bad = gap > tl[ar, best] + tl[ar, got]
        assert not bad.any(), (what, r0 + np.nonzero(~nan)[0][bad][:5], got[bad][:5], best[bad][:5], gap[bad][:5])
        tied = gap == 0
        assert (got[tied] == best[tied]).all(), (what, "tie", r0 + np.nonzero(~nan)[0][tied & (got != best)][:5])


def probed_lists(queries, centroids, nprobe):
    """query -> its nprobe lists [Q, nprobe], by the float64 ranking of the centroids against the f32 query.  Asserts that
    the ranking is the f32 search's too: the nprobe-th score exceeds the next by more than four times the larger tolerance."""
    q, c = np.asarray(queries, dtype=np.float32).astype(np.float64), centroids.astype(np.float64)
    ex = q @ c.T
    tl = TOL * (np.abs(q) @ np.abs(c).T)
    order = np.argsort(-ex, axis=1, kind="stable")
    if nprobe < len(c):
        ar = np.arange(len(q))
        a, b = order[:, nprobe - 1], order[:, nprobe]
        gap, need = ex[ar, a] - ex[ar, b], 4 * np.maximum(tl[ar, a], tl[ar, b])
        assert (gap > need).all(), ("probe margin", nprobe, np.nonzero(gap <= need)[0], gap.min())
    return order[:, :nprobe]


def permitted_rows(lists, live, probe):
    """[Q, N] bool: live rows whose list is probed, plus live tail rows (list -1)"""
    lists = np.asarray(lists)
    per = np.stack([np.isin(lists, p) for p in probe])               # (a probed list id is never -1)
    return (per | (lists == -1)[None, :]) & live[None, :]


def cross_check_by_filter(ix, queries, permitted, k):
    """the documented contract, through the public calls: per query one search with exactly its permitted rows allowed"""
    ids = np.empty((len(queries), k), np.int32)
    sc = np.empty((len(queries), k), np.float32)
    for i, q in enumerate(queries):
        ids[i], sc[i] = (a[0] for a in ix.search(q[None], k, allow=permitted[i]))
    return ids, sc


# ---- data whose lists are known by construction

def sign_centroids(rng, n_lists, dim):
    """n_lists distinct sign patterns over sqrt(dim): unit centroids any two of which differ in the sign of an element"""
    if dim <= 16:
        assert n_lists <= 2 ** dim
        codes = rng.choice(2 ** dim, n_lists, replace=False)
        bits = (codes[:, None] >> np.arange(dim)[None, :]) & 1
    else:
        bits = rng.integers(0, 2, (n_lists, dim))
        assert len(np.unique(bits, axis=0)) == n_lists
    return (np.where(bits > 0, 1.0, -1.0) / np.sqrt(dim)).astype(np.float32)


def rows_around(rng, centroids, of):
    """row i: the unit vector of centroid of[i] with every element scaled by a factor in [0.7, 1.3].  The signs are the
    centroid's, in every stored form (the smallest element is more than half the largest: no i8 code is 0), so the row's score
    against another centroid is its own minus twice a sum of positive terms: its list is of[i], in exact arithmetic by
    at least 2 * 0.7 / (1.3 * dim) of margin (one differing sign) — check_lists and the callers' asserts hold the GPU to it."""
    c = centroids[of]
    return unit(c * (1 + 0.3 * rng.uniform(-1, 1, c.shape)).astype(np.float32))


def lengths_layout(rng, lengths):
    """of [sum(lengths)]: list l has lengths[l] rows, shuffled"""
    of = np.repeat(np.arange(len(lengths)), lengths)
    return of[rng.permutation(len(of))]


def candidates(rng, Q, n_cand, n_rows, holes):
    """[Q, n_cand] distinct ids per query, a tenth of the entries -1 if holes (test_gpu_rescore.py)"""
    cand = np.stack([rng.permutation(n_rows)[:n_cand] for _ in range(Q)]).astype(np.int32)
    if holes:
        cand[rng.random(cand.shape) < 0.1] = -1
    return cand
