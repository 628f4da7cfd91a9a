"""Ordered score sequences for the selecting kernels, and a host model of their candidate queue.  Nothing here touches the GPU or
calls the library: test_topk_order_host.py proves on the CPU that each fixture reaches the queue state it is meant to reach, and
test_gpu_topk_order.py runs the same fixtures through index_topk_kernel, index_probe_kernel, topk_merge_kernel (search.hip) and
sparse_index_scan_kernel (sparse_index.hip), test_gpu_token_index_order.py the token fixtures through token_index_scan_kernel
(token_index.hip), test_gpu_token_scan_forms.py the int8, masked and listed token fixtures through that kernel's other four
instantiations, test_gpu_hybrid_order.py the hybrid fixtures — a dense and a sparse index that carry one pattern together or alone —
through sparse_hybrid_scan_kernel (sparse_index.hip) behind index_scores_kernel and mask_and_kernel (search.hip),
test_gpu_sparse_inverted_order.py the sparse fixtures through sparse_postings_scan_kernel (sparse_postings.hip) under the geometries of
INVERTED_CELLS, which test_sparse_inverted_order_host.py proves on the CPU.

The kernels select alike.  A query's current top-k stands in slots [0, k) of an LDS list of L entries; a (score, id) threshold — the
k-th best at the last sort, (-inf, INT_MAX) before the first — lives in registers; every row that ranks before the threshold is
pushed behind slot k; the lists of a workgroup are sorted, and the thresholds refreshed, only when some query's count exceeds
room = L - k - step, step being the most pushes between two checks.  So k + room + step = L with nothing to spare: a step that
ends with count == room is not sorted, and the next one may push up to slot L - 1.

Scores.  Every value is a non-negative integer that f16 holds exactly (VALUES: 0 .. 2048, then every 2nd, 4th, ... up to 65504),
named by its rank: rank 0 is the value 0, a larger rank a larger value.  A row carries one value per pattern, a query selects one
of them with weight +1 or -1 or selects nothing, so a score is one product by +-1 and sums of zeros: exact in f16 and f32 in every
accumulation order.  The quantized forms (i8: one nonzero column per row; b1: the first rank bits set, against an all-ones query)
keep the ORDER of the ranks, and index_reference.exact_scores states their bits."""
import numpy as np

import index_reference as ixr
import sparse_index_reference as sref

SENT = 2 ** 31 - 1                      # id of an empty list entry (score -inf)
QT = 32                                 # queries of a dense tile
DENSE_STEP, SPARSE_STEP = 128, 256      # rows per step
TOKEN_STEP = 64                         # documents per step of token_index_scan_kernel: 16 rounds of its four waves
MERGE_STEP, MERGE_L, MERGE_OUTER = 256, 512, 4096
PROBE_CHUNK = 1024                      # rows of a tail chunk of the probed search


def dense_L(k):
    """entries of a list of index_topk_kernel and index_probe_kernel"""
    return 256 if k <= 128 else 512


def sparse_L(k):
    return 512 if k <= 128 else 1024


def token_L(k):
    """entries of the list of token_index_scan_kernel (token_index_kernels.h token_list_L)"""
    return 256 if k + TOKEN_STEP <= 256 else 512


_ints = np.arange(65505, dtype=np.float32)
VALUES = _ints[_ints.astype(np.float16).astype(np.float32) == _ints]      # ascending; VALUES[r] == r for r <= 2048


def values(ranks):
    return VALUES[np.asarray(ranks, dtype=np.int64)]


# ------------------------------------------------------------------------------------------------
# patterns: ranks [n] as functions of the row id
# ------------------------------------------------------------------------------------------------
def ascending(n, base=0):
    """every row beats everything before it.  (Descending is the same rows under the negated query, constant the zero query: all
    ties, only the k smallest ids may come back.)"""
    return base + 1 + np.arange(n)


def sawtooth(n, step):
    """period 2 * step; the teeth repeat their values, so later teeth tie with earlier ones and lose by id"""
    return 1 + np.arange(n) % (2 * step)


def fit_schedule(n, k, L, step, lead, extra=0):
    """push [n] bool — the rows that are to enter the queue: `lead` steps of all rows, then cycles of (exactly room = L - k - step rows
    packed into as few steps as take them, then a whole step).  A queue that was emptied in front of a cycle so ends a step with
    count == room, is not sorted, and takes a full step behind it: up to slot L - 1.  room == 0: the cycle is (a step of no row, a whole
    step).  extra = 1: room + 1 rows — one more than fits, so the step must be sorted; a kernel that did not would write slot L."""
    room = L - k - step
    assert room >= 0 and lead >= 0
    out = np.ones((n + step - 1) // step * step + 2 * L + 2 * step, dtype=bool)
    pos = lead * step
    room += extra
    while pos < n:
        if room == 0:
            out[pos:pos + step] = False
            pos += step
        else:
            pos += room // step * step
            p = room % step
            if p:
                out[pos:pos + step] = False
                out[pos + np.arange(p) * step // p] = True         # p rows spread over the step's waves
                pos += step
        pos += step
    return out[:n]


def staircase_lead(k, L, step):
    """the steps of all-pushing rows after which a sort has left k rows in the list, so that the threshold in the registers is a row's.
    Where the first sort already sees k rows (room + step >= k: every dense, sparse and merge geometry) that is the first sort,
    (L - k - step) // step + 1 steps; a short step (the token scan: 64 rows against k up to 256) sorts several times before."""
    room = L - k - step
    assert room >= 0
    held = cnt = lead = 0
    while held < k:
        lead += 1
        cnt += step
        if cnt > room:
            held, cnt = min(k, held + cnt), 0
    return lead


def staircase(n, k, L, step, extra=0):
    """the exact-fit pattern of the unmasked kernels: the rows of fit_schedule that push are ascending, the others have rank 0 — below
    the threshold that the first sort (at the end of the lead) left in the registers.  extra = 1: the near miss, one row more than fits"""
    push = fit_schedule(n, k, L, step, staircase_lead(k, L, step), extra)
    return np.where(push, np.cumsum(push), 0)


def fit_mask(n, k, L, step, extra=0):
    """the exact-fit pattern of the masked kernels, over ascending rows: the rows that are not to push are removed or disallowed, so
    the first cycle runs while the thresholds are still -inf.  Two rows near the end are masked in any case (k + step == L - step has
    a schedule of all rows).  extra = 1: the near miss, as staircase's."""
    ok = fit_schedule(n, k, L, step, 0, extra).copy()
    ok[[n - 1, max(0, n - 3)]] = False
    return ok


# ------------------------------------------------------------------------------------------------
# the queue model
# ------------------------------------------------------------------------------------------------
def _better(s, i, ts, ti):
    return (s > ts) | ((s == ts) & (i < ti))


def walk(scores, ids, ok, k, L, step, slack=0, forget=0):
    """One workgroup: scores [nq, n] f32 of its nq queries against its n rows in the order it meets them, ids [n], ok [n] or [nq, n]
    (False: the row is removed, disallowed or an empty entry, and never pushed).  Pushes and sorts only.  Returns
      steps, sorts (not counting the one behind the last step), sort_steps (the steps that ended in a sort),
      max_slot (the largest slot written; -1: none), fit_fresh / fit_stale [nq] (a step ended with count == room, unsorted, and the next
      step pushed `step` rows — before / after the workgroup's first sort), near_miss [nq] (a step ended with count == room + 1, was
      sorted, and the next step pushed `step` rows), pushed_late [nq] (a push after the first sort),
      ids / scores [nq, k] (the lists at the end, best first; SENT / -inf where empty).
    slack is 0 for every kernel.  slack > 0 is a deliberately WRONG queue, for test_topk_order_host.py's sensitivity checks alone: it
    sorts only when a count exceeds room + slack, and a push behind slot L - 1 — the list has L entries — is lost.  forget > 0 is
    another WRONG queue, for test_sparse_inverted_order_host.py's: at the start of every forget-th step — a segment edge of
    sparse_postings_scan_kernel — the counts go back to 0 unsorted, and what stood behind the top-k is lost."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nq, n = scores.shape
    ids = np.asarray(ids, dtype=np.int64)
    ok = np.ascontiguousarray(np.broadcast_to(np.asarray(ok, dtype=bool), (nq, n)))
    room = L - k - step
    assert room >= 0 and ids.shape == (n,)
    # (equal queries walk alike, and a sort is the workgroup's: on any query's count)
    seen, first, inverse = {}, [], []
    for q in range(nq):
        u = seen.setdefault(scores[q].tobytes() + ok[q].tobytes(), len(first))
        if u == len(first):
            first.append(q)
        inverse.append(u)
    inverse = np.array(inverse, dtype=np.int64)
    U = len(first)
    top_s = [np.empty(0, np.float32) for _ in range(U)]
    top_i = [np.empty(0, np.int64) for _ in range(U)]
    que_s = [[] for _ in range(U)]
    que_i = [[] for _ in range(U)]
    ts, ti = np.full(U, -np.inf, np.float32), np.full(U, SENT, np.int64)
    cnt, prev_fit = np.zeros(U, np.int64), np.zeros(U, bool)
    fit_fresh, fit_stale, late = np.zeros(U, bool), np.zeros(U, bool), np.zeros(U, bool)
    near, prev_over = np.zeros(U, bool), np.zeros(U, bool)
    sorts, max_slot, sort_steps = 0, -1, []
    if room == 0:
        prev_fit[:] = True                                           # (an empty queue is a full one)

    def sort_all():
        for u in range(U):
            s = np.concatenate([top_s[u]] + que_s[u])
            i = np.concatenate([top_i[u]] + que_i[u])
            order = np.lexsort((i, -s.astype(np.float64)))[:k]
            top_s[u], top_i[u] = s[order], i[order]
            que_s[u], que_i[u] = [], []
            if len(order) == k:
                ts[u], ti[u] = top_s[u][-1], top_i[u][-1]
        cnt[:] = 0

    n_steps = (n + step - 1) // step
    for t in range(n_steps):
        sl = slice(t * step, min(n, (t + 1) * step))
        if forget and t and t % forget == 0:                         # (the wrong queue: the edge forgets what was not sorted)
            que_s, que_i = [[] for _ in range(U)], [[] for _ in range(U)]
            cnt[:] = 0
            prev_fit[:] = room == 0
        for u in range(U):
            s, i = scores[first[u], sl], ids[sl]
            m = ok[first[u], sl] & _better(s, i, ts[u], ti[u])
            pushed = int(m.sum())
            if slack and pushed > L - k - int(cnt[u]):               # (the wrong queue: what does not fit is lost)
                m[np.flatnonzero(m)[L - k - int(cnt[u]):]] = False
                pushed = int(m.sum())
            if pushed:
                que_s[u].append(s[m])
                que_i[u].append(i[m])
                cnt[u] += pushed
                max_slot = max(max_slot, k + int(cnt[u]) - 1)
                late[u] |= sorts > 0
            if prev_fit[u] and pushed == step:
                (fit_stale if sorts > 0 else fit_fresh)[u] = True
            if prev_over[u] and pushed == step:
                near[u] = True
        assert max_slot < L, "the model's own invariant: k + room + step == L"
        prev_over = cnt == room + 1                                  # (more than fits: sorted below)
        if (cnt > room + slack).any():
            sort_all()
            sorts += 1
            sort_steps.append(t)
        prev_fit = cnt == room
    if cnt.any():
        sort_all()
    out_i = np.full((U, k), SENT, np.int64)
    out_s = np.full((U, k), -np.inf, np.float32)
    for u in range(U):
        out_i[u, :len(top_i[u])], out_s[u, :len(top_s[u])] = top_i[u], top_s[u]
    return dict(steps=n_steps, sorts=sorts, sort_steps=sort_steps, max_slot=max_slot, L=L, room=room,
                fit_fresh=fit_fresh[inverse], fit_stale=fit_stale[inverse], near_miss=near[inverse], pushed_late=late[inverse],
                ids=out_i[inverse], scores=out_s[inverse])


def merge(list_s, list_i, k):
    """topk_merge_kernel over the candidates [nq, n_cand] of each query (one workgroup per query): rounds of 256 pushes behind a top-k in
    a list of 512, outer rounds of 4096 candidates.  Returns the walks (one per query) and the result (ids -1 where empty)."""
    nq, n_cand = list_s.shape
    cache, walks = {}, []
    for q in range(nq):
        key = list_s[q].tobytes() + list_i[q].tobytes()
        if key not in cache:
            cache[key] = walk(list_s[q][None], list_i[q], list_i[q] != SENT, k, MERGE_L, MERGE_STEP)
        walks.append(cache[key])
    ids = np.concatenate([w["ids"] for w in walks])
    sc = np.concatenate([w["scores"] for w in walks])
    return dict(walks=walks, rounds=(n_cand + MERGE_OUTER - 1) // MERGE_OUTER, n_cand=n_cand,
                ids=np.where(ids == SENT, -1, ids).astype(np.int32), scores=sc)


def sliced_search(S, ok, k, tile, slices, slice_rows, L, step):
    """index_topk_kernel (tile 32, step 128), sparse_index_scan_kernel or sparse_hybrid_scan_kernel (tile qb, step 256), or
    sparse_postings_scan_kernel (tile qb, step 256, slice_rows = slice_segs * seg: postings_search below) over S [nq, n]: one walk per
    (slice, tile of queries), then the merge of the slices' lists.  Returns wgs (the walks), merge (as merge()), ids / scores [nq, k]."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    nq, n = S.shape
    ok = np.broadcast_to(np.asarray(ok, dtype=bool), (nq, n))
    assert (slices - 1) * slice_rows < max(n, 1) <= slices * slice_rows and slice_rows % step == 0
    list_s = np.full((nq, slices, k), -np.inf, np.float32)
    list_i = np.full((nq, slices, k), SENT, np.int64)
    wgs, cache = [], {}
    for sl in range(slices):
        r0, r1 = sl * slice_rows, min(n, (sl + 1) * slice_rows)
        for q0 in range(0, nq, tile):
            key = (sl, S[q0:q0 + tile, r0:r1].tobytes(), ok[q0:q0 + tile, r0:r1].tobytes())
            if key not in cache:                                     # (tiles of the same queries walk alike)
                cache[key] = walk(S[q0:q0 + tile, r0:r1], np.arange(r0, r1), ok[q0:q0 + tile, r0:r1], k, L, step)
            w = dict(cache[key])
            w["q0"], w["slice"] = q0, sl
            wgs.append(w)
            list_s[q0:q0 + tile, sl], list_i[q0:q0 + tile, sl] = w["scores"], w["ids"]
    m = merge(list_s.reshape(nq, -1), list_i.reshape(nq, -1), k)
    return dict(wgs=wgs, merge=m, ids=m["ids"], scores=m["scores"], slices=slices)


def probed_search(S, ok, k, lists, n_lists):
    """index_probe_kernel with every list probed, in list order (the centroid scores of the fixtures tie, so the probe order is the
    ids'): per query one walk per list — its members in ascending id — and per 1024-row chunk of the tail (lists == -1, the rows behind
    the partition), then the merge of the items' lists.  Returns as sliced_search, wgs[item] holding the walks of the unique queries."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    nq, n = S.shape
    ok = np.broadcast_to(np.asarray(ok, dtype=bool), (nq, n))
    lists = np.asarray(lists)
    n_part = int((lists >= 0).sum())
    assert (lists[:n_part] >= 0).all() and (lists[n_part:] == -1).all()
    items = [np.nonzero(lists == l)[0] for l in range(n_lists)]
    items += [np.arange(t0, min(n, t0 + PROBE_CHUNK)) for t0 in range(n_part, n, PROBE_CHUNK)]
    L = dense_L(k)
    list_s = np.full((nq, len(items), k), -np.inf, np.float32)
    list_i = np.full((nq, len(items), k), SENT, np.int64)
    wgs = []
    for it, members in enumerate(items):
        if len(members) == 0:
            wgs.append(None)                                         # (an empty list: k empty entries, no walk)
            continue
        cache, parts = {}, []
        for q in range(nq):                                          # one workgroup per (query, item): no sort is shared
            key = S[q, members].tobytes() + ok[q, members].tobytes()
            if key not in cache:
                cache[key] = walk(S[q:q + 1, members], members, ok[q:q + 1, members], k, L, DENSE_STEP)
            parts.append(cache[key])
        w = dict(parts[0])
        for f in ("fit_fresh", "fit_stale", "near_miss", "pushed_late", "ids", "scores"):
            w[f] = np.concatenate([p[f] for p in parts])
        for f in ("sorts", "max_slot"):
            w[f] = max(p[f] for p in parts)
        wgs.append(w)
        list_s[:, it], list_i[:, it] = w["scores"], w["ids"]
    m = merge(list_s.reshape(nq, -1), list_i.reshape(nq, -1), k)
    return dict(wgs=wgs, merge=m, ids=m["ids"], scores=m["scores"], items=items)


def reference_topk(S, ok, k):
    """the order rule over the permitted rows (index_reference.ref_topk): what every search of S must return"""
    S = np.array(S, dtype=np.float32)
    S[~np.broadcast_to(np.asarray(ok, dtype=bool), S.shape)] = np.nan
    return ixr.ref_topk(S, k)


# ------------------------------------------------------------------------------------------------
# the tiles of a fixture: which query stands where
# ------------------------------------------------------------------------------------------------
def layouts(kinds, busy, idle, nq, tile):
    """name -> [nq] kinds.  "first:b" / "last:b": the first / last query of every tile is the busy kind b (for each of busy) and its
    neighbours push nothing after their first k rows; "mixed": every kind in turn."""
    out = {}
    for b in busy:
        for name in ("first", "last"):
            lay = [idle[i % len(idle)] for i in range(nq)]
            for q0 in range(0, nq, tile):
                lay[q0 if name == "first" else min(nq, q0 + tile) - 1] = b
            if lay not in out.values():
                out[f"{name}:{b}"] = lay
    lay = [kinds[i % len(kinds)] for i in range(nq)]
    if lay not in out.values():
        out["mixed"] = lay
    return out


class Fixture:
    """One index and its queries by kind.  scores[kind] [n] f32 are the reference's (the stored form's rule), intended[kind] [n] the
    signed values the pattern means, ok [n] the rows a search may return (None: all), ok1 a second allow-list (the near miss of ok's
    exact fit; None where ok is), busy / idle the kinds of layouts()."""

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def S(self, layout):
        return np.stack([self.scores[kind] for kind in layout])

    def permitted(self):
        return np.ones(self.n, dtype=bool) if self.ok is None else self.ok


def check_order(scores, intended, what=""):
    """the reference's scores are a strictly increasing function of the intended values: equal where those are equal, ordered as they
    are"""
    order = np.lexsort((np.arange(len(intended)), intended))
    s, v = scores[order].astype(np.float64), np.asarray(intended, dtype=np.float64)[order]
    assert not np.isnan(s).any(), what
    assert ((np.diff(s) > 0) == (np.diff(v) > 0)).all() and (np.diff(s) >= 0).all(), what


# ------------------------------------------------------------------------------------------------
# dense fixtures: index_topk_kernel
# ------------------------------------------------------------------------------------------------
DENSE_DTYPES = ixr.DTYPES
DENSE_KS = (1, 127, 128, 129, 256)
DENSE_NQS = (1, 31, 32, 33)
DENSE_ROWS = {"f32": 2500, "f16": 2500, "i8": 2500, "b1": 2040}       # 19 whole steps and 68 rows; b1: 15 and 120 (its ranks end at dim)
MODES = ("plain", "removed", "allow")
B1_DIM = 2048
FLOAT_DIM = 8


def dense_rows(dtype, patterns):
    """rows [n, dim] f32 that carry the rank patterns: a column each (f32, f16), the one pattern in column 0 (i8: one nonzero column
    per row, so its scale cannot reorder the pattern), or the first rank bits set (b1)"""
    n = len(patterns[0])
    if dtype == "b1":
        assert len(patterns) == 1 and patterns[0].max() <= B1_DIM
        return np.where(np.arange(B1_DIM)[None, :] < patterns[0][:, None], np.float32(1), np.float32(-1))
    assert len(patterns) <= FLOAT_DIM and (dtype != "i8" or len(patterns) == 1)
    rows = np.zeros((n, FLOAT_DIM), np.float32)
    for c, ranks in enumerate(patterns):
        rows[:, c] = values(ranks)
    return rows


def dense_query(dtype, col, sign):
    """+-e_col, or the zero vector (sign 0); b1: +-(all ones) — the only query that orders its rows"""
    q = np.zeros(B1_DIM if dtype == "b1" else FLOAT_DIM, np.float32)
    if dtype == "b1":
        q[:] = sign
    else:
        q[col] = sign
    return q


def dense_scores(dtype, queries, rows):
    """[Q, n] f32 by the reference of the stored form: bit for bit where index_reference restates the integer arithmetic (i8, b1), the
    float64 score of the stored values otherwise — which the callers assert to be the intended integers, exact in f32"""
    if dtype in ("i8", "b1"):
        return ixr.exact_scores(queries, rows, dtype)
    exact = ixr.FloatScores(queries, rows, dtype).exact
    assert (exact == exact.astype(np.float32)).all()
    return exact.astype(np.float32) + np.float32(0)                  # (a zero score is +0: the chain starts at +0)


def _dense_fixture(name, dtype, patterns, names, ok, busy):
    """patterns: rank arrays; names: per pattern (kind of +, kind of -)"""
    rows = dense_rows(dtype, patterns)
    n = len(rows)
    kinds, intended = {"const": dense_query(dtype, 0, 0)}, {"const": np.zeros(n)}
    for c, (ranks, (pos, neg)) in enumerate(zip(patterns, names)):
        v = values(ranks).astype(np.float64)
        if dtype == "b1":
            v = 2.0 * ranks - B1_DIM                                 # (set bits minus clear bits)
        kinds[pos], intended[pos] = dense_query(dtype, c, 1), v
        kinds[neg], intended[neg] = dense_query(dtype, c, -1), -v
    order = list(kinds)
    sc = dense_scores(dtype, np.stack([kinds[kk] for kk in order]), rows)
    scores = {kk: sc[i] for i, kk in enumerate(order)}
    for kk in order:
        if dtype in ("f32", "f16"):
            assert np.array_equal(scores[kk].astype(np.float64), intended[kk]), (name, kk)       # exactly the intended integers
        else:
            check_order(scores[kk], intended[kk], (name, kk))
    if dtype == "f32":
        chain = ixr.f32_chain_scores(np.stack([kinds[kk] for kk in order]), rows)                 # the documented fma chain agrees
        assert np.array_equal(chain.view(np.uint32), sc.view(np.uint32)), name
    idle = [kk for kk in ("const", "desc") if kk in kinds]
    return Fixture(name, dtype=dtype, rows=rows, n=n, queries=kinds, scores=scores, intended=intended, ok=ok, kinds=order,
                   busy=busy, idle=idle)


def dense_fixtures(dtype, k, mode):
    """The indexes of one (dtype, k, mode) cell.  plain: ascending, sawtooth, the unmasked exact-fit staircase of this k and its near
    miss.  removed /
    allow: ascending and sawtooth under fit_mask(k), the masked exact fit (the ascending rows that must not push are removed or
    disallowed).  f32 and f16 hold the patterns side by side in one index; i8 and b1 hold one pattern per index."""
    n, L, step = DENSE_ROWS[dtype], dense_L(k), DENSE_STEP
    pats = [(ascending(n), ("asc", "desc"), "asc"), (sawtooth(n, step), ("saw", "was"), "saw")]
    ok = ok1 = None
    if mode == "plain":
        pats.append((staircase(n, k, L, step), ("stair", "riats"), "stair"))
        pats.append((staircase(n, k, L, step, 1), ("over", "revo"), "over"))
    else:
        ok, ok1 = fit_mask(n, k, L, step), fit_mask(n, k, L, step, 1)
    if dtype in ("f32", "f16"):
        out = [_dense_fixture(f"{dtype} k={k} {mode}", dtype, [p[0] for p in pats], [p[1] for p in pats], ok, ["stair", "over", "asc"] if mode == "plain" else ["asc"])]
    else:
        out = [_dense_fixture(f"{dtype} k={k} {mode} {p[2]}", dtype, [p[0]], [p[1]], ok, [p[2]]) for p in pats]
    for fx in out:
        fx.ok1 = ok1
    return out


# ------------------------------------------------------------------------------------------------
# many slices (f32): the merge's outer rounds and its refill
# ------------------------------------------------------------------------------------------------
MANY_DENSE_ROWS = 17 * 4096
MANY_SPARSE_ROWS = 17 * 2048
MANY_NQS = (1, 33)
MANY_KS = (256, 10)


def many_scores(n):
    """kind -> scores [n]: plain integers (exact in f32 up to 2^24) ascending over the whole index — every slice beats all earlier ones,
    so the merge refills in every round —, descending, constant"""
    v = (1 + np.arange(n)).astype(np.float32)
    return {"asc": v, "desc": -v, "const": np.zeros(n, np.float32)}


MANY_LAYOUT = ["asc", "desc", "const"]


def many_layout(nq):
    return [MANY_LAYOUT[i % 3] for i in range(nq)]


# ------------------------------------------------------------------------------------------------
# the merge's own exact fit: a rescore hands topk_merge_kernel its candidates in the caller's order
# ------------------------------------------------------------------------------------------------
MERGE_CAND = 1024                        # the most candidates of a rescore: four rounds of the merge
MERGE_KS = DENSE_KS
MERGE_KINDS = ["stair", "riats", "over", "revo", "const"]


def merge_scores(k):
    """kind -> scores [1024] of rows 0 .. 1023, which a rescore names in this order: the staircase of the merge's geometry (a round of
    all candidates, then room = 512 - k - 256 of them and a whole round) and its near miss"""
    st = values(staircase(MERGE_CAND, k, MERGE_L, MERGE_STEP))
    ov = values(staircase(MERGE_CAND, k, MERGE_L, MERGE_STEP, 1))
    return {"stair": st, "riats": -st + np.float32(0), "over": ov, "revo": -ov + np.float32(0), "const": np.zeros(MERGE_CAND, np.float32)}


MERGE_COLUMN = {"stair": (0, 1.0), "riats": (0, -1.0), "over": (1, 1.0), "revo": (1, -1.0), "const": (-1, 0.0)}


# ------------------------------------------------------------------------------------------------
# probed fixtures: index_probe_kernel
# ------------------------------------------------------------------------------------------------
PROBE_LISTS = 4
PROBE_LONG = 1600                        # members of list 0: 12 whole steps and 64 rows
PROBE_SHORT = 150                        # members of lists 1 and 2; list 3 is empty
PROBE_TAIL = 1100                        # rows added after the partition: two chunks
PROBE_KS = DENSE_KS
PROBE_BIG = 64.0                         # the list's axis of a row; i8: every pattern value is larger, so a row's scale is its value / 127


PROBE_FORMS = ("stair", "over", "allow")


def probe_fixture(dtype, k, form):
    """Centroids on separate axes (e_0 .. e_3); row = big * e_list + value * e_last (b1: the list's bit, and the first rank bits behind
    the list columns), so list membership is by construction and the query e_last (b1: ones behind the list columns) scores the pattern
    alone — 0 against every centroid, so with nprobe = n_lists no probe ranking is in question.  The long list holds the unmasked
    staircase of k ("stair"), its near miss ("over") or ascending rows under fit_mask ("allow") in ascending member order, interleaved in storage with two short lists of
    sawtooth rows; the tail is ascending.  Returns the Fixture with lists [n] (-1: the tail), centroids, n_part."""
    L, step, masked = dense_L(k), DENSE_STEP, form == "allow"
    n_part = PROBE_LONG + 2 * PROBE_SHORT
    n = n_part + PROBE_TAIL
    # storage order of the partitioned rows: a short-list row after every 5th or 6th long-list row
    lists = np.zeros(n_part, np.int64)
    at = np.linspace(3, n_part - 2, 2 * PROBE_SHORT).astype(np.int64)
    assert len(np.unique(at)) == len(at)
    lists[at] = 1 + np.arange(len(at)) % 2
    lists = np.concatenate([lists, np.full(PROBE_TAIL, -1)])
    long_rows = np.nonzero(lists == 0)[0]
    assert len(long_rows) == PROBE_LONG
    base = 80 if dtype == "i8" else 0                                # i8: values above PROBE_BIG
    ranks = np.zeros(n, np.int64)
    ok = ok1 = None
    if masked:
        ranks[long_rows] = base + ascending(PROBE_LONG)
        ok = np.ones(n, dtype=bool)
        ok1 = ok.copy()
        ok[long_rows], ok1[long_rows] = fit_mask(PROBE_LONG, k, L, step), fit_mask(PROBE_LONG, k, L, step, 1)
        for m in (ok, ok1):
            m[[n - 1, n_part + 5, n_part + 40]] = False              # tail rows too: one word, and a block that straddles two
    else:
        st = staircase(PROBE_LONG, k, L, step, int(form == "over"))
        ranks[long_rows] = np.where(st > 0, base + st, 0)
    for l in (1, 2):
        ranks[lists == l] = base + sawtooth(PROBE_SHORT, 16)
    # the tail goes on ascending above the long list (b1: its ranks end at the dim, so the tail starts over and ties with the list)
    ranks[n_part:] = (0 if dtype == "b1" else base + PROBE_LONG) + ascending(PROBE_TAIL)
    if dtype == "b1":
        dim, P0 = B1_DIM, PROBE_LISTS
        assert ranks.max() <= dim - P0
        col = np.arange(dim)[None, :]
        bits = (col >= P0) & (col < P0 + ranks[:, None])
        bits |= (col == np.where(lists >= 0, lists, 0)[:, None]) & (lists >= 0)[:, None]
        rows = np.where(bits, np.float32(1), np.float32(-1))
        q = np.zeros(dim, np.float32)
        q[P0:] = 1
        v = 2.0 * ranks - (dim - P0)
    else:
        dim = FLOAT_DIM
        rows = np.zeros((n, dim), np.float32)
        rows[:, dim - 1] = values(ranks)
        part = np.nonzero(lists >= 0)[0]
        rows[part, lists[part]] = PROBE_BIG
        q = np.zeros(dim, np.float32)
        q[dim - 1] = 1
        v = values(ranks).astype(np.float64)
    centroids = np.zeros((PROBE_LISTS, dim), np.float32)
    centroids[np.arange(PROBE_LISTS), np.arange(PROBE_LISTS)] = 1
    kinds = {"pattern": q, "inverse": -q, "const": np.zeros(dim, np.float32)}
    intended = {"pattern": v, "inverse": -v, "const": np.zeros(n)}
    order = list(kinds)
    sc = dense_scores(dtype, np.stack([kinds[kk] for kk in order]), rows)
    scores = {kk: sc[i] for i, kk in enumerate(order)}
    name = f"probe {dtype} k={k} {form}"
    for kk in order:
        if dtype in ("f32", "f16"):
            assert np.array_equal(scores[kk].astype(np.float64), intended[kk]), (name, kk)
        elif dtype == "b1":
            check_order(scores[kk], intended[kk], (name, kk))
        else:
            # i8: a tail row (one nonzero column) and a list row (two) of one value may differ in the last bit of their scales'
            # product; the order is asked of the rows of each item, whose rows are built alike
            for sel in (lists == 0, lists == 1, lists == 2, lists == -1):
                check_order(scores[kk][sel], intended[kk][sel], (name, kk))
    return Fixture(name, dtype=dtype, rows=rows, n=n, queries=kinds, scores=scores, intended=intended, ok=ok, kinds=order,
                   ok1=ok1, busy=["pattern"], idle=["const"], lists=lists, centroids=centroids, n_part=n_part, long_rows=long_rows)


def probe_layout(nq=3):
    return ["pattern", "inverse", "const"][:nq]


# ------------------------------------------------------------------------------------------------
# sparse fixtures: sparse_index_scan_kernel
# ------------------------------------------------------------------------------------------------
SPARSE_DTYPES = ["f32", "f16"]
SPARSE_KS = (1, 127, 128, 129, 255, 256)
SPARSE_ROWS = 4000                       # 15 whole steps and 160 rows
SPARSE_V = 1000
SPARSE_TERMS = {"asc": (0, 1.0), "desc": (0, -1.0), "saw": (1, 1.0), "was": (1, -1.0), "stair": (2, 1.0), "riats": (2, -1.0), "over": (3, 1.0), "revo": (3, -1.0),
                "const": (-1, 0.0)}


def sparse_query(kinds):
    """(ids [nq, 1], weights [nq, 1]): a query holds the one term id of its pattern with weight +-1, or no term"""
    ids = np.array([[SPARSE_TERMS[kk][0]] for kk in kinds], np.int32)
    w = np.array([[SPARSE_TERMS[kk][1]] for kk in kinds], np.float32)
    return ids, w


def sparse_fixture(dtype, k, mode, n=SPARSE_ROWS):
    """One index: row r holds term p with the value of pattern p's rank — 0 ascending, 1 sawtooth, 2 (plain) the unmasked staircase of
    k, 3 its near miss —, and a query holds one of the ids with weight +-1: the score is fmaf(w, +-1, +0), the stored weight or its negation.  removed /
    allow: fit_mask(k)."""
    L, step = sparse_L(k), SPARSE_STEP
    pats = [ascending(n), sawtooth(n, step)]
    ok = ok1 = None
    if mode == "plain":
        pats += [staircase(n, k, L, step), staircase(n, k, L, step, 1)]
    else:
        ok, ok1 = fit_mask(n, k, L, step), fit_mask(n, k, L, step, 1)
    ids = np.tile(np.arange(len(pats), dtype=np.int32), (n, 1))
    w = np.stack([values(p) for p in pats], axis=1).astype(np.float32)
    st = sref.stored_rows(ids, w, len(pats), dtype)
    assert np.array_equal(st[1], w)                                  # (f16 holds every value)
    order = [kk for kk, (t, _) in SPARSE_TERMS.items() if t < len(pats)]
    sc = sref.scores(st[0], st[1], *sparse_query(order), SPARSE_V)
    scores = {kk: sc[i] for i, kk in enumerate(order)}
    name = f"sparse {dtype} k={k} {mode}"
    for kk in order:
        t, sign = SPARSE_TERMS[kk]
        want = np.zeros(n) if t < 0 else sign * w[:, t].astype(np.float64)
        assert np.array_equal(scores[kk].astype(np.float64), want), (name, kk)
    return Fixture(name, dtype=dtype, n=n, term_ids=ids, term_w=w, scores=scores, ok=ok, ok1=ok1, kinds=order, width=len(pats),
                   busy=["stair", "over", "asc"] if mode == "plain" else ["asc"], idle=["const", "desc"])


def many_sparse_rows(n=MANY_SPARSE_ROWS):
    """rows of width 1: term 0 with weight 1 + r (f32)"""
    return np.zeros((n, 1), np.int32), (1 + np.arange(n)).astype(np.float32)[:, None]


# ------------------------------------------------------------------------------------------------
# hybrid fixtures: sparse_hybrid_scan_kernel (sparse_index.hip), behind index_scores_kernel and mask_and_kernel (search.hip)
# ------------------------------------------------------------------------------------------------
# A hybrid fixture is a dense and a sparse index of equal size and queries by kind (the kinds of SPARSE_TERMS).  The intended hybrid score
# of row r under a kind is +- values(rank_p(r)), the patterns those of the sparse fixtures: the scan's geometry, steps of 256 rows and
# sparse_L(k) entries.  scores[kind] is hybrid_reference.combine(D, S, w_dense, w_sparse) of the two stored forms' reference scores D
# (index_reference) and S (sparse_index_reference).  The carrier says which side holds the pattern:
#   split   both: lo = B * ((v // B) mod C) with (B, C) = HYBRID_SPLIT — the middle digit of v in the mixed radix (B, C) — under the sparse
#           term id, hi = v - lo — the top and the bottom digit — in the dense column, each divided by the size of its weight.  All weights
#           are powers of two, so both products and their sum are exact: H = +-v bit for bit (but for the sign of a zero).  Neither side
#           alone, nor the weights swapped, orders the rows as H does (test_topk_order_host.py; v mod 64, a dense part that dominates the
#           sparse one, does not meet that: 7808, the largest value, stands alone in its block of 64, and swapping (-0.5, -4) stretches
#           the dense part further, which keeps H's order).  A negative pair turns asc into desc without negating a query.
#   dense   the dense index holds the whole pattern (any of the four dtypes), the sparse query holds no term: S = +0, weights (1, 1)
#   sparse  the sparse index holds the whole pattern, the dense query is the zero vector: D = +0, weights (1, 1)
HYBRID_WEIGHTS = ((1.0, 1.0), (2.0, 0.5), (-1.0, -1.0), (-0.5, -4.0))
HYBRID_SPLIT = (24, 16)
HYBRID_ROWS = {"f32": SPARSE_ROWS, "f16": SPARSE_ROWS, "i8": SPARSE_ROWS, "b1": 2040}       # b1: 7 whole steps and 248 rows (its ranks end at dim)
HYBRID_KS = SPARSE_KS
HYBRID_NQS = (1, 2, 3, 5)
HYBRID_DENSE_KS = (1, 128, 129, 256)     # the dense carrier's
HYBRID_DENSE_NQS = (1, 33)               # 33: two dense tiles, the second of one query, and chunks of 32 + 1
HYBRID_SPARSE_KS = (128, 256)            # the sparse carrier's
HYBRID_CHUNK = 2                         # the value of "hybrid_chunk_queries" in the chunked case: 5 queries are chunks of 2, 2 and 1
HYBRID_CHUNK_NQ, HYBRID_CHUNK_K = 5, 128
HYBRID_PATTERN_KINDS = [("asc", "desc"), ("saw", "was"), ("stair", "riats"), ("over", "revo")]
OPPOSITE = {a: b for pair in HYBRID_PATTERN_KINDS for a, b in (pair, pair[::-1])}
OPPOSITE["const"] = "const"
_HYBRID_FIXTURES = {}


def hybrid_patterns(n, k, mode):
    """(ranks of pattern 0 .. [n] each, ok, ok1) of one (k, mode) cell, as sparse_fixture's: ascending, sawtooth, and (plain) the
    staircase of (k, sparse_L(k), 256) and its near miss, or (removed / allow) fit_mask and its near miss"""
    L, step = sparse_L(k), SPARSE_STEP
    pats = [ascending(n), sawtooth(n, step)]
    ok = ok1 = None
    if mode == "plain":
        pats += [staircase(n, k, L, step), staircase(n, k, L, step, 1)]
    else:
        ok, ok1 = fit_mask(n, k, L, step), fit_mask(n, k, L, step, 1)
    return pats, ok, ok1


def masked_reaches_stale(n, k):
    """whether the masked exact fit over n ascending rows also fits exactly behind a sort (fit_stale), not only before the first one:
    2040 rows end before the second such cycle at k = 129 and 255 (test_topk_order_host.py walks every k at both sizes)"""
    return not (n == 2040 and k in (129, 255))


def _hybrid_fixture(name, wd, ws, positive, plain, **kw):
    """the Fixture of one pair of indexes: scores = H under (wd, ws); effective[kind] is the kind whose intended scores H[kind] are —
    the kind itself, or its opposite where the weights are negative; busy / idle are query kinds by what H does"""
    import hybrid_reference as href

    fx = Fixture(name, w=(wd, ws), **kw)
    fx.scores = {kk: href.combine(fx.dsc[kk], fx.ssc[kk], wd, ws) for kk in fx.kinds}
    fx.effective = {kk: kk if positive else OPPOSITE[kk] for kk in fx.kinds}
    by = {e: kk for kk, e in fx.effective.items()}
    fx.busy = [by[e] for e in (("stair", "over", "asc") if plain else ("asc",)) if e in by]
    fx.idle = [by[e] for e in ("const", "desc") if e in by]
    for d in (fx.dsc, fx.ssc, fx.scores):
        for a in d.values():
            a.setflags(write=False)
    for a in (fx.rows, fx.term_ids, fx.term_w, fx.ok, fx.ok1):
        if a is not None:
            a.setflags(write=False)
    return fx


def hybrid_queries(fx, lay):
    """(dense queries [nq, dim] f32, q_ids [nq, 1], q_w [nq, 1]) of a layout of kinds"""
    ids = np.array([[fx.sparse_q[kk][0]] for kk in lay], np.int32)
    w = np.array([[fx.sparse_q[kk][1]] for kk in lay], np.float32)
    return np.stack([fx.dense_q[kk] for kk in lay]), ids, w


def hybrid_split_fixture(dd, sd, k, mode, weights, n=SPARSE_ROWS, split=None):
    """The split carrier of one (k, mode) cell under one weight pair (dd in f32, f16).  Asserts what makes it exact: every stored value
    survives f16, the dense reference's scores are +-hi / |w_dense| exactly (f32: the documented fma chain agrees), the sparse reference's
    +-lo / |w_sparse|, and (w_dense * D) + (w_sparse * S) == +-v in float32 — equal values, hence equal bits but for the sign of a zero."""
    split = HYBRID_SPLIT if split is None else split
    key = ("split", dd, sd, k, mode, weights, n, split)
    if key in _HYBRID_FIXTURES:
        return _HYBRID_FIXTURES[key]
    assert dd in ("f32", "f16")
    wd, ws = weights
    assert (wd > 0) == (ws > 0) and wd != 0
    sgn = 1.0 if wd > 0 else -1.0
    pats, ok, ok1 = hybrid_patterns(n, k, mode)
    P = len(pats)
    v = np.stack([values(p) for p in pats], axis=1).astype(np.float32)                            # [n, P]
    lo = np.float32(split[0]) * np.mod(np.floor(v / np.float32(split[0])), np.float32(split[1]))
    hi = v - lo
    rows = np.zeros((n, FLOAT_DIM), np.float32)
    rows[:, :P] = hi / np.float32(abs(wd))
    term_ids = np.tile(np.arange(P, dtype=np.int32), (n, 1))
    term_w = lo / np.float32(abs(ws))
    name = f"hybrid split {dd} x {sd} k={k} {mode} w=({wd:g}, {ws:g})"
    for a in (rows, term_w):
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a), name                   # (both stored forms hold every value)
    kinds = [kk for kk, (t, _) in SPARSE_TERMS.items() if t < P]
    dense_q = {kk: dense_query(dd, max(SPARSE_TERMS[kk][0], 0), SPARSE_TERMS[kk][1]) for kk in kinds}
    sparse_q = {kk: SPARSE_TERMS[kk] for kk in kinds}
    dq = np.stack([dense_q[kk] for kk in kinds])
    Dm = dense_scores(dd, dq, rows)
    if dd == "f32":
        assert np.array_equal(ixr.f32_chain_scores(dq, rows).view(np.uint32), Dm.view(np.uint32)), name
    st = sref.stored_rows(term_ids, term_w, P, sd)
    assert np.array_equal(st[1], term_w), name
    Sm = sref.scores(st[0], st[1], *sparse_query(kinds), SPARSE_V)
    D, S, intended = {}, {}, {}
    for i, kk in enumerate(kinds):
        t, sign = SPARSE_TERMS[kk]
        D[kk], S[kk] = Dm[i], Sm[i]
        want_d = np.zeros(n) if t < 0 else sign * rows[:, t].astype(np.float64)
        want_s = np.zeros(n) if t < 0 else sign * term_w[:, t].astype(np.float64)
        assert np.array_equal(D[kk].astype(np.float64), want_d) and np.array_equal(S[kk].astype(np.float64), want_s), (name, kk)
        intended[kk] = np.zeros(n) if t < 0 else sgn * sign * v[:, t].astype(np.float64)
    fx = _hybrid_fixture(name, wd, ws, wd > 0, mode == "plain", carrier="split", dd=dd, sd=sd, k=k, mode=mode, n=n, rows=rows,
                         term_ids=term_ids, term_w=term_w, width=P, dense_q=dense_q, sparse_q=sparse_q, dsc=D, ssc=S, intended=intended,
                         ok=ok, ok1=ok1, kinds=kinds, split=split)
    for kk in kinds:
        assert np.array_equal(fx.scores[kk].astype(np.float64), intended[kk]), (name, kk)         # H is the intended value itself
    assert max(np.abs(a).max() for a in fx.scores.values()) == v.max() <= 7808
    _HYBRID_FIXTURES[key] = fx
    return fx


def hybrid_dense_fixtures(dd, sd, k, mode):
    """The dense carrier of one (k, mode) cell: the index pairs (f32, f16: one, the patterns side by side; i8, b1: one per pattern) whose
    dense rows are dense_rows(dd, patterns), whose sparse rows are the sparse fixture's and whose sparse queries hold no term.  D is the
    exact integers (f32, f16) or index_reference.exact_scores (i8, b1); S = +0; H = D + (+0) under (1, 1)."""
    key = ("dense", dd, sd, k, mode)
    if key in _HYBRID_FIXTURES:
        return _HYBRID_FIXTURES[key]
    n = HYBRID_ROWS[dd]
    pats, ok, ok1 = hybrid_patterns(n, k, mode)
    names = HYBRID_PATTERN_KINDS[:len(pats)]
    term_ids = np.tile(np.arange(len(pats), dtype=np.int32), (n, 1))
    term_w = np.stack([values(p) for p in pats], axis=1).astype(np.float32)
    st = sref.stored_rows(term_ids, term_w, len(pats), sd)
    groups = [(pats, names)] if dd in ("f32", "f16") else [([p], [nm]) for p, nm in zip(pats, names)]
    out = []
    for gp, gn in groups:
        name = f"hybrid dense {dd} x {sd} k={k} {mode}" + ("" if len(groups) == 1 else f" {gn[0][0]}")
        base = _dense_fixture(name, dd, gp, gn, ok, [])
        kinds = base.kinds
        none = np.full((len(kinds), 1), -1, np.int32), np.zeros((len(kinds), 1), np.float32)
        Sm = sref.scores(st[0], st[1], *none, SPARSE_V)
        assert not Sm.any() and not np.signbit(Sm).any(), name
        fx = _hybrid_fixture(name, 1.0, 1.0, True, mode == "plain", carrier="dense", dd=dd, sd=sd, k=k, mode=mode, n=n, rows=base.rows,
                             term_ids=term_ids, term_w=term_w, width=len(pats), dense_q=base.queries, sparse_q={kk: (-1, 0.0) for kk in kinds},
                             dsc=base.scores, ssc={kk: Sm[i] for i, kk in enumerate(kinds)}, intended=base.intended, ok=ok, ok1=ok1, kinds=kinds)
        for kk in kinds:
            assert np.array_equal(fx.scores[kk], fx.dsc[kk]), (name, kk)                              # D + (+0) == D
        out.append(fx)
    _HYBRID_FIXTURES[key] = out
    return out


def hybrid_sparse_fixture(dd, sd, k, mode="plain"):
    """The sparse carrier (dd in f32, f16): the sparse index is sparse_fixture's, the dense rows hold the same patterns and every dense
    query is the zero vector: D = +0, H = (+0) + S under (1, 1)"""
    key = ("sparse", dd, sd, k, mode)
    if key in _HYBRID_FIXTURES:
        return _HYBRID_FIXTURES[key]
    assert dd in ("f32", "f16")
    base = sparse_fixture(sd, k, mode)
    n, kinds = base.n, base.kinds
    pats, ok, ok1 = hybrid_patterns(n, k, mode)
    rows = dense_rows(dd, pats)
    zero = dense_query(dd, 0, 0)
    name = f"hybrid sparse {dd} x {sd} k={k} {mode}"
    Dm = dense_scores(dd, np.stack([zero] * len(kinds)), rows)
    assert not Dm.any() and not np.signbit(Dm).any(), name
    fx = _hybrid_fixture(name, 1.0, 1.0, True, mode == "plain", carrier="sparse", dd=dd, sd=sd, k=k, mode=mode, n=n, rows=rows,
                         term_ids=base.term_ids, term_w=base.term_w, width=base.width, dense_q={kk: zero for kk in kinds},
                         sparse_q={kk: SPARSE_TERMS[kk] for kk in kinds}, dsc={kk: Dm[i] for i, kk in enumerate(kinds)},
                         ssc=dict(base.scores), intended={kk: base.scores[kk].astype(np.float64) for kk in kinds}, ok=ok, ok1=ok1, kinds=kinds)
    for kk in kinds:
        assert np.array_equal(fx.scores[kk], fx.ssc[kk]), (name, kk)                                  # (+0) + S == S
    _HYBRID_FIXTURES[key] = fx
    return fx


def hybrid_reference(fx, k, ok=None):
    """kind -> hybrid_reference.search of the fixture's D and S under its weights over the rows that qualify (ok: another set than the
    fixture's), (ids [1, k], scores [1, k]); made once per (k, set)"""
    import hybrid_reference as href

    qual = fx.permitted() if ok is None else np.asarray(ok, dtype=bool)
    cache = fx.__dict__.setdefault("_reference", {})
    key = (k, qual.tobytes())
    if key not in cache:
        cache[key] = {kk: href.search(fx.dsc[kk][None], fx.ssc[kk][None], qual, fx.w[0], fx.w[1], k) for kk in fx.kinds}
    return cache[key]


def of_layout(want, lay):
    """the per-kind results of a layout of kinds, stacked"""
    return np.concatenate([want[kk][0] for kk in lay]), np.concatenate([want[kk][1] for kk in lay])


def hybrid_removed_split(ok, three_ways):
    """(ids removed from the dense index, ids removed from the sparse index, the allow-list or None) that leave exactly the rows ok:
    the others by r % 3 — dense, sparse, disallowed: mask_and_kernel's AND of three inputs — or all of them removed in the sparse
    index alone"""
    gone = np.flatnonzero(~ok)
    if not three_ways:
        return np.zeros(0, np.int32), gone.astype(np.int32), None
    allow = np.ones(len(ok), dtype=bool)
    allow[gone[gone % 3 == 2]] = False
    parts = gone[gone % 3 == 0].astype(np.int32), gone[gone % 3 == 1].astype(np.int32), allow
    assert all(len(p) > 0 for p in parts[:2])                        # (k = 256 masks two rows only: the allow-list is then all ones)
    live = np.ones(len(ok), dtype=bool)
    live[parts[0]] = False
    live[parts[1]] = False
    assert np.array_equal(live & allow, ok)
    return parts


def hybrid_chunks(n, nq, pref, hook):
    """[(c0, c)] of a call of nq queries, from the library's own rule (hook = pybert.test_hybrid_chunk), and ld"""
    hc, ld = hook(n, nq, pref)
    assert ld == (n + 63) // 64 * 64 and hc >= 1
    return [(c0, min(hc, nq - c0)) for c0 in range(0, nq, hc)], ld


def many_hybrid_rows(n=MANY_SPARSE_ROWS):
    """(dense rows [n, 8] f32, term ids [n, 1], term weights [n, 1]): 1 + r split at 64 between column 0 and term 0 — plain integers,
    exact in f32, so H = many_scores(n) under (1, 1)"""
    v = 1 + np.arange(n)
    rows = np.zeros((n, FLOAT_DIM), np.float32)
    rows[:, 0] = 64 * (v // 64)
    return rows, np.zeros((n, 1), np.int32), (v % 64).astype(np.float32)[:, None]


def many_hybrid_fixture(n=MANY_SPARSE_ROWS):
    """the f32 x f32 pair of many slices and its kinds asc / desc / const: D and S by the two references, H == many_scores(n)"""
    key = ("many", n)
    if key in _HYBRID_FIXTURES:
        return _HYBRID_FIXTURES[key]
    rows, term_ids, term_w = many_hybrid_rows(n)
    kinds = list(MANY_LAYOUT)
    dense_q = {kk: dense_query("f32", 0, SPARSE_TERMS[kk][1]) for kk in kinds}
    sparse_q = {kk: SPARSE_TERMS[kk] for kk in kinds}
    Dm = dense_scores("f32", np.stack([dense_q[kk] for kk in kinds]), rows)
    st = sref.stored_rows(term_ids, term_w, 1, "f32")
    Sm = sref.scores(st[0], st[1], *sparse_query(kinds), SPARSE_V)
    fx = _hybrid_fixture(f"hybrid many {n}", 1.0, 1.0, True, True, carrier="split", dd="f32", sd="f32", n=n, rows=rows, term_ids=term_ids,
                         term_w=term_w, width=1, dense_q=dense_q, sparse_q=sparse_q, dsc={kk: Dm[i] for i, kk in enumerate(kinds)},
                         ssc={kk: Sm[i] for i, kk in enumerate(kinds)}, ok=None, ok1=None, kinds=kinds)
    sc = many_scores(n)
    for kk in kinds:
        assert np.array_equal(fx.scores[kk], sc[kk]), kk
    _HYBRID_FIXTURES[key] = fx
    return fx


# ------------------------------------------------------------------------------------------------
# token fixtures: token_index_scan_kernel (token_index.hip)
# ------------------------------------------------------------------------------------------------
TOKEN_KS =(1, 64, 128, 129, 191, 192, 193, 255, 256)
TOKEN_DOCS = TOKEN_STEP * 24 + 37        # 24 whole steps and a tail that ends inside a step and inside a group of four waves
TOKEN_DIM = 8
TOKEN_DOC_LENS = (1, 31, 32, 33, 65)     # by document id: the masked last block of 32 document tokens is in play
TOKEN_QUERY_LENS = (1, 33)               # the first token selects; zero rows behind it: a second query block that adds +0
TOKEN_COLUMN = {"asc": (0, 1.0), "desc": (0, -1.0), "saw": (1, 1.0), "was": (1, -1.0), "stair": (2, 1.0), "riats": (2, -1.0), "over": (3, 1.0),
                "revo": (3, -1.0), "const": (-1, 0.0)}
TOKEN_KINDS = list(TOKEN_COLUMN)
TOKEN_MANY_SLICES, TOKEN_MANY_K = 17, 256
TOKEN_MANY_DOCS = 3301                   # 17 slices of 195 documents (the last: 181): 3 steps and 3 documents, 48 groups of four and 3


def token_search(S, k, n_slices, slice_docs, ok=True):
    """token_index_scan_kernel over S [nq, n_docs]: one walk per (query, slice of slice_docs consecutive documents; the last takes what
    is left, and a slice need not be whole steps), steps of TOKEN_STEP documents from the slice's first, then the merge of the slices'
    lists.  The order of the pushes inside a step — the four waves' atomicAdd — is not modelled: walk() sorts by (score, id) alone.
    ok [n_docs]: the documents that qualify (live and allowed), the masked instantiations' step mask.  The masked kernel skips its look at
    the count behind a step without a qualifying document; walk() looks and needs no change for that: nothing was pushed in such a step,
    so the count is what the last look left, which was <= room (a larger one was sorted and reset), and the look it skips finds nothing.
    Returns as sliced_search."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    nq, n = S.shape
    assert (n_slices - 1) * slice_docs < max(n, 1) <= n_slices * slice_docs
    ok = np.ascontiguousarray(np.broadcast_to(np.asarray(ok, dtype=bool), (n,)))
    L = token_L(k)
    list_s = np.full((nq, n_slices, k), -np.inf, np.float32)
    list_i = np.full((nq, n_slices, k), SENT, np.int64)
    wgs, cache = [], {}
    for sl in range(n_slices):
        r0, r1 = sl * slice_docs, min(n, (sl + 1) * slice_docs)
        for q in range(nq):
            key = (sl, S[q, r0:r1].tobytes())
            if key not in cache:
                cache[key] = walk(S[q:q + 1, r0:r1], np.arange(r0, r1), ok[r0:r1], k, L, TOKEN_STEP)
            w = dict(cache[key])
            w["q0"], w["slice"] = q, sl
            wgs.append(w)
            list_s[q, sl], list_i[q, sl] = w["scores"][0], w["ids"][0]
    m = merge(list_s.reshape(nq, -1), list_i.reshape(nq, -1), k)
    return dict(wgs=wgs, merge=m, ids=m["ids"], scores=m["scores"], slices=n_slices)


def token_fixture(k, n=TOKEN_DOCS):
    """One token index of n documents and its queries by kind.  Document d is TOKEN_DOC_LENS[d % 5] copies of one row that carries the
    value of pattern p's rank in column p — 0 ascending, 1 sawtooth of period 128, 2 the staircase of (k, token_L(k), 64), 3 its near
    miss —; a query's first token is +-e_p (or zero), the tokens behind it are zero rows.  A score is so one product by +-1, a max over
    equal values and sums of zeros: scores[kind] [n] f32 are exact in any order.  An unmasked slot behind a document's end would enter
    the max as 0 and beat every score of a negated pattern.
    rows [T, 8] f32, cu [n + 1]; queries(kinds, lens) packs a query set."""
    L = token_L(k)
    pats = [ascending(n), sawtooth(n, TOKEN_STEP), staircase(n, k, L, TOKEN_STEP), staircase(n, k, L, TOKEN_STEP, 1)]
    per_doc = np.zeros((n, TOKEN_DIM), np.float32)
    for c, ranks in enumerate(pats):
        per_doc[:, c] = values(ranks)
    assert np.array_equal(per_doc.astype(np.float16).astype(np.float32), per_doc)                 # (the index stores f16)
    lens = np.array([TOKEN_DOC_LENS[d % len(TOKEN_DOC_LENS)] for d in range(n)], np.int64)
    rows = np.repeat(per_doc, lens, axis=0)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    scores = {}
    for kk, (col, sign) in TOKEN_COLUMN.items():
        scores[kk] = np.zeros(n, np.float32) if col < 0 else np.float32(sign) * per_doc[:, col] + np.float32(0)
    return Fixture(f"token k={k} n={n}", n=n, k=k, rows=rows, cu=cu, lens=lens, scores=scores, kinds=TOKEN_KINDS)


def token_queries(kinds, lens):
    """(rows [T, 8] f32, cu int32) of one query per (kind, len) pair: +-e_col, then len - 1 zero rows"""
    parts = []
    for kk, ln in zip(kinds, lens):
        q = np.zeros((ln, TOKEN_DIM), np.float32)
        col, sign = TOKEN_COLUMN[kk]
        if col >= 0:
            q[0, col] = sign
        parts.append(q)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


def token_layout():
    """every kind at every query length: (kinds, lens)"""
    kinds = [kk for kk in TOKEN_KINDS for _ in TOKEN_QUERY_LENS]
    return kinds, [ln for _ in TOKEN_KINDS for ln in TOKEN_QUERY_LENS]


def token_scores_f64(fx, kinds, lens):
    """[nq, n] float64 by the definition, from the rows themselves: sum over the query's tokens of the max over the document's tokens of
    the dot product (what scores[kind] states in closed form)"""
    q, qcu = token_queries(kinds, lens)
    out = np.zeros((len(kinds), fx.n))
    prod = q.astype(np.float64) @ fx.rows.astype(np.float64).T                                    # [query tokens, document tokens]
    mx = np.maximum.reduceat(prod, fx.cu[:-1], axis=1)                                            # per document
    for i in range(len(kinds)):
        out[i] = mx[qcu[i]:qcu[i + 1]].sum(axis=0)
    return out


# ------------------------------------------------------------------------------------------------
# int8 token fixtures: token_index_scan_kernel<I8Form, ...>
# ------------------------------------------------------------------------------------------------
TOKEN_I8_SIGN = {"asc": 1.0, "desc": -1.0, "saw": 1.0, "was": -1.0, "stair": 1.0, "riats": -1.0, "over": 1.0, "revo": -1.0, "const": 0.0}
TOKEN_I8_PATTERNS = {"asc": ("asc", "desc"), "saw": ("saw", "was"), "stair": ("stair", "riats"), "over": ("over", "revo")}
_I8_FIXTURES = {}


def token_i8_queries(kinds, lens):
    """(rows [T, 8] f32, cu int32) of one query per (kind, len) pair: +-e_0 or a zero row, then len - 1 zero rows"""
    parts = []
    for kk, ln in zip(kinds, lens):
        q = np.zeros((ln, TOKEN_DIM), np.float32)
        q[0, 0] = TOKEN_I8_SIGN[kk]
        parts.append(q)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


def token_i8_rows(ranks):
    """(rows [T, 8] f32, cu int32, lens): document d is TOKEN_DOC_LENS[d % 5] copies of value(ranks[d]) * e_0 — one nonzero column, so a
    token's scale is its value / 127 and its code 127: no other column is there for the scale to round away"""
    n = len(ranks)
    per_doc = np.zeros((n, TOKEN_DIM), np.float32)
    per_doc[:, 0] = values(ranks)
    lens = np.array([TOKEN_DOC_LENS[d % len(TOKEN_DOC_LENS)] for d in range(n)], np.int64)
    return np.repeat(per_doc, lens, axis=0), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), lens


def _token_i8_fixture(name, ranks, pos, neg):
    """One int8 token index over the ranks [n] and its queries by kind (pos: +e_0, neg: -e_0, "const": zero).  scores[kind] [n] f32 are
    token_i8_reference.scores_i8 of the rows themselves — the bits the index must give —, asserted to be the same at both query lengths
    (the zero rows behind the first token add +0) and to keep the ranks' order exactly (check_order).  Under neg every score of a positive
    rank is negative, so an unmasked slot behind a document's end (0) would beat it.  Made once, read-only."""
    import token_i8_reference as t8

    if name in _I8_FIXTURES:
        return _I8_FIXTURES[name]
    ranks = np.asarray(ranks, dtype=np.int64)
    n = len(ranks)
    rows, cu, lens = token_i8_rows(ranks)
    kinds = [pos, neg, "const"]
    q, qcu = token_i8_queries([kk for kk in kinds for _ in TOKEN_QUERY_LENS], [ln for _ in kinds for ln in TOKEN_QUERY_LENS])
    sc = t8.scores_i8(q, qcu, rows, cu)
    v = values(ranks).astype(np.float64)
    scores, intended = {}, {pos: v, neg: -v, "const": np.zeros(n)}
    for i, kk in enumerate(kinds):
        a, b = sc[2 * i], sc[2 * i + 1]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.signbit(a[a == 0]).any(), (name, kk)
        check_order(a, intended[kk], (name, kk))
        scores[kk] = a
    for a in (rows, cu, lens, ranks, *scores.values()):
        a.setflags(write=False)
    fx = Fixture(name, n=n, rows=rows, cu=cu, lens=lens, ranks=ranks, scores=scores, intended=intended, kinds=kinds, pos=pos, neg=neg)
    _I8_FIXTURES[name] = fx
    return fx


def token_i8_fixture(pattern, k=None, n=TOKEN_DOCS):
    """The int8 index of one pattern: "asc", "saw" (period 128), "stair" (the staircase of (k, token_L(k), 64)) or "over" (its near miss)"""
    pos, neg = TOKEN_I8_PATTERNS[pattern]
    if pattern == "asc":
        return _token_i8_fixture(f"token i8 asc n={n}", ascending(n), pos, neg)
    if pattern == "saw":
        return _token_i8_fixture(f"token i8 saw n={n}", sawtooth(n, TOKEN_STEP), pos, neg)
    return _token_i8_fixture(f"token i8 {pattern} k={k} n={n}", staircase(n, k, token_L(k), TOKEN_STEP, int(pattern == "over")), pos, neg)


def token_i8_layout(fx):
    """every kind of the fixture at every query length: (kinds, lens)"""
    return [kk for kk in fx.kinds for _ in TOKEN_QUERY_LENS], [ln for _ in fx.kinds for ln in TOKEN_QUERY_LENS]


# ------------------------------------------------------------------------------------------------
# masked token fixtures, both forms: token_index_scan_kernel<Form, true, false>
# ------------------------------------------------------------------------------------------------
TOKEN_MASK_MODES = ("allow", "removed", "both")
TOKEN_MASK_KINDS = ["asc", "desc", "const"]
TOKEN_MASK_SLICES = (1, 0, 7)            # one slice; the planned cut; 7 slices, which start inside a mask word


def token_masks(k, n=TOKEN_DOCS):
    """(ok, ok1) [n] bool over the ascending pattern: the masked exact fit of this k and its near miss"""
    L = token_L(k)
    return fit_mask(n, k, L, TOKEN_STEP), fit_mask(n, k, L, TOKEN_STEP, 1)


def token_mask_mode(ok, mode):
    """(the ids to remove, the allow-list or None) that leave exactly the documents ok: as an allow-list, as removals, or as both — a
    random half of the others removed, the rest disallowed"""
    if mode == "allow":
        return np.zeros(0, np.int32), ok
    if mode == "removed":
        return np.flatnonzero(~ok).astype(np.int32), None
    r = np.random.default_rng(len(ok)).random(len(ok)) < 0.5
    removed, allow = np.flatnonzero(~(ok | r)).astype(np.int32), ok | ~r
    live = np.ones(len(ok), dtype=bool)
    live[removed] = False
    assert np.array_equal(live & allow, ok)
    return removed, allow


# ------------------------------------------------------------------------------------------------
# listed fixtures: token_index_scan_kernel<I8Form, false, true>, the int8 rescore
# ------------------------------------------------------------------------------------------------
LIST_DOCS = MERGE_CAND                   # document d has rank d: its id is its rank, and document 0 scores 0
LIST_HOLES = (-1, LIST_DOCS, 2 ** 31 - 1, None)       # what stands at a hole, in turn; None: the position's own id, removed from the index


def listed_fixture():
    return _token_i8_fixture(f"token i8 ids n={LIST_DOCS}", np.arange(LIST_DOCS), "asc", "desc")


def candidate_lists(k):
    """name -> (cand [1024] int64, removed ids): candidate lists that carry a pattern along their POSITIONS.
      arange        position == id: ascending
      reversed      the ids descend, so under "desc" the scores ascend along the positions while the ids fall
      holes         ascending, with a hole wherever fit_mask(k) says "no push": the masked exact fit (thresholds still -inf).  The holes are
                    LIST_HOLES in turn: -1, n_docs, 2^31 - 1, and ids that are removed from the index
      holes over    its near miss
      repeats       the ids are the staircase's ranks: the exact fit behind a stale threshold; every position that is not to push names
                    document 0, whose score 0 is the best of all under "desc" — as often as it is named
      repeats over  its near miss"""
    n, L = LIST_DOCS, token_L(k)
    none = np.zeros(0, np.int32)
    out = {"arange": (np.arange(n), none), "reversed": (n - 1 - np.arange(n), none)}
    for name, extra in (("holes", 0), ("holes over", 1)):
        cand, removed = np.arange(n), []
        ok = fit_mask(n, k, L, TOKEN_STEP, extra)
        ok[[n - 2, n - 4]] = False                                   # (at least four holes, one of each kind, where the schedule is all rows)
        for j, p in enumerate(np.flatnonzero(~ok)):
            h = LIST_HOLES[j % len(LIST_HOLES)]
            if h is None:
                removed.append(p)
            else:
                cand[p] = h
        out[name] = (cand, np.array(removed, np.int32))
    for name, extra in (("repeats", 0), ("repeats over", 1)):
        cand = staircase(n, k, L, TOKEN_STEP, extra).astype(np.int64)
        cand[[n - 1, n - 2, n - 4]] = 0                              # (document 0 at least three times, where the staircase is all rows)
        out[name] = (cand, none)
    return out


def list_valid(cand, removed, n_docs=LIST_DOCS):
    """the positions that hold a candidate: an id in [0, n_docs) that is not removed"""
    cand = np.asarray(cand, dtype=np.int64)
    return (cand >= 0) & (cand < n_docs) & ~np.isin(cand, removed)


def list_scores(S, cand, removed):
    """S [nq, n_docs] with NaN in the removed documents' columns: what tref.rescore_expected ranks"""
    Sm = np.array(S, dtype=np.float32)
    Sm[:, np.asarray(removed, dtype=np.int64)] = np.nan
    return Sm


def listed_search(S, cand, valid, k, n_slices, slice_pos, positions_for_ids=False, slack=0):
    """the listed instantiation over S [nq, n_docs] and ONE candidate list cand [n_cand] for all queries: one walk per (query, slice of
    slice_pos consecutive POSITIONS), whose rows are the documents cand[r0:r1] in list order under their own ids, valid [n_cand] saying
    which positions hold a candidate; then the merge.  positions_for_ids and slack make deliberately wrong models (the sensitivity
    checks).  Returns as sliced_search."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    nq, n = len(S), len(cand)
    assert (n_slices - 1) * slice_pos < n <= n_slices * slice_pos
    L = token_L(k)
    at = np.where((cand >= 0) & (cand < S.shape[1]), cand, 0)
    list_s = np.full((nq, n_slices, k), -np.inf, np.float32)
    list_i = np.full((nq, n_slices, k), SENT, np.int64)
    wgs, cache = [], {}
    for sl in range(n_slices):
        r0, r1 = sl * slice_pos, min(n, (sl + 1) * slice_pos)
        ids = np.arange(r0, r1) if positions_for_ids else cand[r0:r1]
        for q in range(nq):
            key = (sl, S[q, at[r0:r1]].tobytes())
            if key not in cache:
                cache[key] = walk(S[q:q + 1, at[r0:r1]], ids, valid[r0:r1], k, L, TOKEN_STEP, slack)
            w = dict(cache[key])
            w["q0"], w["slice"] = q, sl
            wgs.append(w)
            list_s[q, sl], list_i[q, sl] = w["scores"][0], w["ids"][0]
    m = merge(list_s.reshape(nq, -1), list_i.reshape(nq, -1), k)
    return dict(wgs=wgs, merge=m, ids=m["ids"], scores=m["scores"], slices=n_slices)


# ------------------------------------------------------------------------------------------------
# inverted fixtures: sparse_postings_scan_kernel (sparse_postings.hip)
# ------------------------------------------------------------------------------------------------
# The inverted scan selects with the row-major scan's constants (steps of 256 rows, sparse_L(k) entries, the same sort trigger), but its
# workgroup walks a slice of whole SEGMENTS and carries the thresholds, the counts and the queue over every segment edge, with the
# accumulators zeroed in between.  Its fixtures are the sparse ones (sparse_fixture, many_sparse_rows); what is new is the geometry they
# run under: the segment size ("sparse_index_segment_rows", read by invert), the number of queries (which decides how many segments a
# workgroup walks) and the tile ("sparse_index_qb").  INVERTED_CELLS lists every (seg, nq, tile key, k, mode) that
# test_gpu_sparse_inverted_order.py runs with what the cell is there to reach; test_sparse_inverted_order_host.py proves each claim
# with the plan's hook and the model.
INVERTED_QCHUNK = 4096                   # queries per internal pass (sparse_index.h SparseIndex::QCHUNK)
INVERTED_LDS_STATIC = 65536              # what a kernel gets without hipFuncSetAttribute
INVERTED_ONE_SEG = 4096                  # the 4000-row fixtures are one (partial) segment
INVERTED_NQS = (1, 2, 3, 5)
INVERTED_WALKED = ((256, 4096), (1024, 4096), (256, 4097), (1024, 4097), (256, 600))          # (seg, nq)
INVERTED_WALKED_KS = (1, 128, 129, 256)
INVERTED_TILES = (1, 2, 3, 4, 8)
INVERTED_TILE_SEGS = (256, 4096)
INVERTED_TILE_K = 128
INVERTED_BIG_ROWS = 16384 + 300          # two segments of 16384 rows, three of 8192
INVERTED_BIG = ((16384, 10, 2), (16384, 256, 2), (8192, 10, 4), (8192, 256, 3))               # (seg, k, the tile under the key 4)
INVERTED_BIG_QB = 4
INVERTED_BIG_NQS = (1, 5, 8)
INVERTED_BIG_GONE = np.arange(16384 - 100, 16384 + 100)                                     # the rows removed around the segment edge


class InvertedCell:
    """One launch geometry of the GPU file.  section: "one" (a single segment), "walked" (a workgroup walks several segments), "tiles".
    reach: the states the cell is there for, each asserted by test_sparse_inverted_order_host.py —
      one_segment      one slice of one segment
      walks_all        the first chunk is ONE slice of all (> 1) segments: every step of seg 256 is a segment edge
      second_chunk     a second chunk of one query, cut into one slice per segment
      several          slice_segs > 1 and n_slices > 1
      short_last       the last slice has fewer segments than the others
      partial_segment  the last segment is partial
      fit              every one-slice workgroup of a busy query ends a step with count == room, unsorted, and pushes a whole step
                       (fresh for the masked modes, stale for plain), up to slot L - 1; the near miss is sorted
      tile=N           the tile the plan gives"""

    def __init__(self, section, seg, nq, qb, k, mode, reach):
        self.section, self.seg, self.nq, self.qb, self.k, self.mode, self.reach = section, seg, nq, qb, k, mode, frozenset(reach)

    def __repr__(self):
        return f"{self.section} seg={self.seg} nq={self.nq} qb={self.qb} k={self.k} {self.mode}"


def _inverted_cells():
    out = []
    for mode in MODES:
        for k in SPARSE_KS:
            for nq in INVERTED_NQS:
                out.append(InvertedCell("one", INVERTED_ONE_SEG, nq, 0, k, mode, {"one_segment", "partial_segment", "fit", f"tile={min(2, nq)}"}))
        for k in INVERTED_WALKED_KS:
            for seg, nq in INVERTED_WALKED:
                reach = {"partial_segment", "tile=2"}
                reach |= {"several", "short_last"} if nq < INVERTED_QCHUNK else {"walks_all", "fit"}
                if nq > INVERTED_QCHUNK:
                    reach |= {"second_chunk"}
                out.append(InvertedCell("walked", seg, nq, 0, k, mode, reach))
    for mode in ("plain", "allow"):
        for seg in INVERTED_TILE_SEGS:
            for n in INVERTED_TILES:
                for nq in sorted({n - 1, n, n + 1, 70} - {0}):
                    reach = {"partial_segment", f"tile={min(n, 4, nq)}"} | ({"one_segment", "fit"} if seg == INVERTED_ONE_SEG else set())
                    out.append(InvertedCell("tiles", seg, nq, n, INVERTED_TILE_K, mode, reach))
    return out


INVERTED_CELLS = _inverted_cells()


def inverted_cells(section, **match):
    return [c for c in INVERTED_CELLS if c.section == section and all(getattr(c, a) == v for a, v in match.items())]


def postings_plan(hook, dtype, n_rows, nq, k, seg, qb=0, n_vocab=SPARSE_V):
    """[(c0, c, g)]: the chunks of a call of nq queries (SparseIndex::QCHUNK) and each chunk's geometry from the library's own plan
    (hook = pybert.test_sparse_postings_geometry), with seg, n_segs and slice_rows added"""
    out = []
    for c0 in range(0, nq, INVERTED_QCHUNK):
        c = min(INVERTED_QCHUNK, nq - c0)
        g = dict(hook(dtype, n_vocab, n_rows, c, k, seg, qb))
        assert g["L"] == sparse_L(k) and seg % SPARSE_STEP == 0
        g["seg"], g["n_segs"], g["slice_rows"] = seg, -(-n_rows // seg), g["slice_segs"] * seg
        out.append((c0, c, g))
    return out


def postings_search(S, ok, k, g):
    """sparse_postings_scan_kernel and the merge over S [nq, n], the queries of ONE chunk under its geometry g (postings_plan): sliced_search
    with the tile, the slices of slice_segs whole segments and the row-major scan's step and list.  A segment is whole steps, so the steps
    of a slice are those of its rows, and a workgroup's thresholds, counts and queue live on over the segment edges."""
    return sliced_search(S, ok, k, g["qb"], g["n_slices"], g["slice_rows"], g["L"], SPARSE_STEP)


def inverted_period(kinds, tile):
    """queries after which the tiles of any layouts() list repeat: a multiple of the tile, of the kinds (mixed) and of the two idle kinds"""
    return tile * len(kinds) * 2


def check_inverted_geometry(cell, n_rows, plan):
    """the geometric claims of a cell on its chunks' geometries"""
    g = plan[0][2]
    n_segs, reach = g["n_segs"], cell.reach
    tile = [int(r.split("=")[1]) for r in reach if r.startswith("tile=")]
    assert len(tile) == 1 and g["qb"] == tile[0] and g["n_qtiles"] == -(-plan[0][1] // tile[0]), (cell, g)
    assert ("one_segment" in reach) == (n_segs == 1) and ("partial_segment" in reach) == (n_rows % cell.seg != 0), (cell, g)
    assert ("walks_all" in reach) == (n_segs > 1 and g["n_slices"] == 1 and g["slice_segs"] == n_segs), (cell, g)
    assert ("several" in reach) == (g["slice_segs"] > 1 and g["n_slices"] > 1), (cell, g)
    assert ("short_last" in reach) == (g["n_slices"] > 1 and n_segs % g["slice_segs"] != 0), (cell, g)
    assert ("second_chunk" in reach) == (len(plan) == 2), (cell, plan)
    if len(plan) == 2:
        c0, c, g1 = plan[1]
        assert (c0, c) == (INVERTED_QCHUNK, 1) and g1["qb"] == 1 and g1["slice_segs"] == 1 and g1["n_slices"] == n_segs > 1, (cell, g1)
    for _, _, gg in plan:
        assert gg["lds"] <= 160 * 1024 - 256 and gg["n_slices"] <= gg["max_slices"], (cell, gg)


def big_inverted_rows(dtype, n=INVERTED_BIG_ROWS):
    """(term ids [n, 1], weights [n, 1], scores by kind) of the large-segment index: term 0 with weight 1 + r (f32: many_sparse_rows) or the
    value of rank 1 + r // 3 (f16: rising in ties of three, inside VALUES); asc / desc / const as many_scores"""
    ids, w = many_sparse_rows(n)
    if dtype == "f16":
        w = values(1 + np.arange(n) // 3)[:, None].astype(np.float32)
        assert np.array_equal(w.astype(np.float16).astype(np.float32), w)
    v = w[:, 0]
    return ids, w, {"asc": v, "desc": -v, "const": np.zeros(n, np.float32)}


# ------------------------------------------------------------------------------------------------
# what a fixture must reach (asserted on the CPU by test_topk_order_host.py)
# ------------------------------------------------------------------------------------------------
def describe(tag, res):
    """one line per fixture for the log: sorts and the largest slot over the scoring workgroups, slices, merge rounds"""
    wgs = [w for w in res["wgs"] if w is not None]
    mw = res["merge"]["walks"]
    return (f"{tag}: workgroups {len(wgs)}, steps {max(w['steps'] for w in wgs)}, sorts {max(w['sorts'] for w in wgs)}, "
            f"largest slot {max(w['max_slot'] for w in wgs)} of L {wgs[0]['L']} (room {wgs[0]['room']}), "
            f"exact fit fresh {int(any(w['fit_fresh'].any() for w in wgs))} stale {int(any(w['fit_stale'].any() for w in wgs))} "
            f"near miss {int(any(w['near_miss'].any() for w in wgs))}; "
            f"merge: candidates {res['merge']['n_cand']}, outer rounds {res['merge']['rounds']}, sorts {max(w['sorts'] for w in mw)}, "
            f"largest slot {max(w['max_slot'] for w in mw)} of {MERGE_L}")
