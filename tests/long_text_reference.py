"""Long texts (bert_hip.h "LONG TEXTS") restated in NumPy: the window plan, the grouped pooling in float64, the derived error
bound of group_pool_kernel (misc_kernels.hip) and an emulation of the kernel's own f32 arithmetic.  No GPU, no library: the host
test holds the emulation to the bound, the GPU test the kernel."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of f32


def f4(a):
    return np.asarray(a, dtype=np.float32)


# ---- the window plan ------------------------------------------------------------------------------------------------------------
def plan_windows(n_tokens, window, stride):
    """The starts, among the INNER ids, of the windows of a text of n_tokens ids ([CLS] ... [SEP]).  window counts all ids of a
    window, stride inner ids.  None for arguments outside n_tokens >= 2, window >= 3, 1 <= stride <= window - 2."""
    if n_tokens < 2 or window < 3 or stride < 1 or stride > window - 2:
        return None
    if n_tokens <= window:
        return [0]
    m, c = n_tokens - 2, window - 2
    starts, s = [], 0
    while s + c < m:
        starts.append(s)
        s += stride
    return starts + [m - c]


def windows_of(ids, window, stride):
    """The windows of a tokenized text as id lists: the text itself if it fits, else [CLS], c inner ids, [SEP] per start"""
    ids = list(ids)
    if len(ids) <= window:
        return [ids]
    inner, c = ids[1:-1], window - 2
    return [[ids[0]] + inner[s:s + c] + [ids[-1]] for s in plan_windows(len(ids), window, stride)]


def pack_groups(texts_windows):
    """[[window ids, ...] per text] -> (packed ids, cu_seqlens, group_cu) as bert_hip_eval_packed_grouped takes them"""
    sents = [w for ws in texts_windows for w in ws]
    cu = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int32)
    group_cu = np.concatenate([[0], np.cumsum([len(ws) for ws in texts_windows])]).astype(np.int32)
    return np.concatenate([np.asarray(s, dtype=np.int32) for s in sents]), cu, group_cu


# ---- grouped pooling ------------------------------------------------------------------------------------------------------------
def group_pool(rows, weights, group_cu, raw):
    """float64: a_g = sum_s w_s r_s / sum_s w_s over the rows group_cu[g] .. group_cu[g + 1] - 1, divided by its L2 norm unless raw"""
    rows = np.asarray(rows, dtype=np.float64)
    w = np.ones(len(rows)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = np.empty((len(group_cu) - 1, rows.shape[1]))
    for g in range(len(group_cu) - 1):
        s0, s1 = int(group_cu[g]), int(group_cu[g + 1])
        a = (w[s0:s1, None] * rows[s0:s1]).sum(axis=0) / w[s0:s1].sum()
        out[g] = a if raw else a / np.sqrt((a * a).sum())
    return out


def group_pool_bound(rows, weights, group_cu, raw):
    """|group_pool_kernel - group_pool| per element, for f32 rows and integer weights, u = 2^-24.

    A group of ONE sentence is copied: raw bound 0 (its normalised form has the norm's terms below alone).

    Raw, a group of S > 1 sentences, element e.  The kernel computes acc = fma(w_S, r_S, ... fma(w_1, r_1, 0)), one rounding per
    step (the products w_s r_s are not rounded: fused), so acc = sum_s w_s r_s (1 + t_s) with |t_s| <= S u to first order
    whatever the signs: S u sum_s w_s |r_s|.  W = sum w is an integer below 2^24, exact in f32; 1 / W rounds once (the division is
    correctly rounded), the product acc (1 / W) once: two more factors (1 + d), |d| <= u, on a value of magnitude at most
    sum_s w_s |r_s| / W.  Together
        B_e = (S + 2) u sum_s w_s |r_s[e]| / W.

    Normalised: out_e = fl(a'_e s'), a' the computed raw row, s' the computed 1 / ||a'||.
      - the sum of squares q' has only positive terms: a thread adds its ceil(H / 256) squares in one fma chain, the wave sum adds
        six times, the four wave sums take two more levels: k = ceil(H / 256) + 8 roundings on the way of any term, q' = ||a'||^2
        (1 + t), |t| <= k u; the square root halves that and rounds once, the reciprocal rounds once, the product with a'_e once:
        |out_e - a'_e / ||a'||| <= (k / 2 + 3) u |a'_e| / ||a'||;
      - the row the kernel normalises is a', not a: |a'_e / ||a'|| - a_e / ||a||| <= |a'_e - a_e| / ||a'|| + |a_e| | ||a'|| -
        ||a|| | / (||a|| ||a'||) <= (B_e + |y_e| ||B||) / ||a'||, y = a / ||a|| the exact result, and ||a'|| >= ||a|| - ||B||.
    So the normalised bound is ((k / 2 + 3) u (|a_e| + B_e) + B_e + |y_e| ||B||) / (||a|| - ||B||).
    The float64 reference's own error (2^-53 per operation) is nine orders of magnitude below u and is left out."""
    rows = np.asarray(rows, dtype=np.float64)
    w = np.ones(len(rows)) if weights is None else np.asarray(weights, dtype=np.float64)
    G, H = len(group_cu) - 1, rows.shape[1]
    bound = np.zeros((G, H))
    want = group_pool(rows, weights, group_cu, True)
    for g in range(G):
        s0, s1 = int(group_cu[g]), int(group_cu[g + 1])
        S = s1 - s0
        if S > 1:
            bound[g] = (S + 2) * U * (w[s0:s1, None] * np.abs(rows[s0:s1])).sum(axis=0) / w[s0:s1].sum()
    if raw:
        return bound
    k = -(-H // 256) + 8
    out = np.zeros((G, H))
    for g in range(G):
        a, B = want[g], bound[g]
        na, nB = np.sqrt((a * a).sum()), np.sqrt((B * B).sum())
        out[g] = ((k / 2 + 3) * U * (np.abs(a) + B) + B + np.abs(a) / na * nB) / (na - nB)
    return out


def _wave_sum(v):
    """wave_sum_f32 on the 64 lane values v (f32): the xor butterfly, distances 32, 16, 8, 4, 2, 1; every lane ends with the sum"""
    v = f4(v).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v = f4(v + v[np.arange(64) ^ o])
    return v[0]


def group_pool_f32(rows, weights, group_cu, raw, drop_last=False, unit_weights=False):
    """group_pool_kernel's own arithmetic in NumPy: thread tid owns elements tid, tid + 256, ...; per element one chain acc = fma(w_s,
    r_s[e], acc) over the group's sentences in ascending order, a = acc * (1 / sum w) with the sum in integers; a group of one sentence
    takes its row unchanged; the norm: per-thread squares in ascending element order, the wave sum, the four partials as (0 + 1) +
    (2 + 3), 1 / sqrtf.  An fma is emulated as the float64 product and sum rounded to f32 once per step: the product of a 10-bit
    weight and an f32 value is exact in float64, the float64 SUM is rounded before it is rounded to f32 again — a double rounding
    that can differ from the device's single one by one f32 ulp of the step in about one case in 2^29: an emulation, not a bit oracle.
    The two wrong kernels the bound must catch: drop_last leaves the group's last sentence out of the chain (not of sum w),
    unit_weights uses w = 1 where token weights are due."""
    rows = f4(rows)
    n, H = rows.shape
    w = np.ones(n, dtype=np.int64) if weights is None or unit_weights else np.asarray(weights, dtype=np.int64)
    out = np.empty((len(group_cu) - 1, H), dtype=np.float32)
    for g in range(len(group_cu) - 1):
        s0, s1 = int(group_cu[g]), int(group_cu[g + 1])
        if s1 - s0 == 1:
            a = rows[s0].copy()
        else:
            acc = np.zeros(H, dtype=np.float32)
            for s in range(s0, s1 - 1 if drop_last else s1):
                acc = f4(np.float64(w[s]) * rows[s].astype(np.float64) + acc.astype(np.float64))
            inv = np.float32(1.0) / np.float32(int(w[s0:s1].sum()))
            a = f4(acc * inv)
        if not raw:
            sq = np.zeros(256, dtype=np.float32)
            for e0 in range(0, H, 256):
                part = np.zeros(256, dtype=np.float32)
                part[:min(256, H - e0)] = a[e0:e0 + 256]
                sq = f4(part.astype(np.float64) * part.astype(np.float64) + sq.astype(np.float64))
            red = [_wave_sum(sq[64 * v:64 * v + 64]) for v in range(4)]
            total = f4(f4(red[0] + red[1]) + f4(red[2] + red[3]))
            a = f4(a * f4(np.float32(1.0) / np.sqrt(total, dtype=np.float32)))
        out[g] = a
    return out


def kernel_case(H, seed=0):
    """The op-level test's input at width H: group sizes [1, 1, 2, 3, 7, 33] in one call, weights 1 .. 512, rows with a mean of their
    own, normal(0.1, 1), and two NaN rows in front of and behind the rows in use.  -> rows [4 + 47][H] f32, weights, group_cu"""
    rng = np.random.default_rng(1000 * seed + H)
    sizes = [1, 1, 2, 3, 7, 33]
    n = sum(sizes)
    rows = np.full((n + 4, H), np.nan, dtype=np.float32)
    rows[2:2 + n] = rng.normal(0.1, 1.0, (n, H))
    weights = np.ones(n + 4, dtype=np.int32)
    weights[2:2 + n] = rng.integers(1, 513, n)
    weights[2], weights[3 + 1] = 512, 1                        # (both ends of the range are there)
    group_cu = (2 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32)
    return rows, weights, group_cu


KERNEL_WIDTHS = (1, 64, 130, 384, 768)
