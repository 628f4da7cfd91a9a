"""Float64 references, derived bounds and case builders for the token rows and the MaxSim score (include/bert_hip.h "token rows
and late interaction"; tests: test_tokens_host.py, test_gpu_tokens.py).  No GPU.

MaxSim.  score(a, b) = sum_i max_j <Q_i, D_j> over the f16-ROUNDED rows, in float64.  The bound, from the arithmetic the header states:
  - an inner product is an f32 accumulation chain: the index tests' own TOL * sum_k |q_k d_k| (index_reference.TOL);
  - the max is exact, so token i's computed maximum differs from the true one by at most the largest tolerance among its candidates
    (every computed product is within its tolerance, and max is monotone): t_i = max_j tol_ij;
  - the f32 sum over the n query tokens: whatever the order, a value passes through at most n - 1 roundings (adding the +0 of a padded
    slot is exact, and a tree over 32 slots is at most 5 deep): gamma(n) * sum_i (|M_i| + t_i);
  - the mean is one more correctly rounded division: U * |score| / n on top of the sum's bound over n.

Token rows.  rows[t] = x[t] / sqrt(sum_e x[t][e]^2) in float64 on the stored values.  The sum of H squares in f32 (H - 1 additions, one
rounding per square), a correctly rounded sqrt (which halves the relative error) and reciprocal, and one multiplication: within
gamma(H + 2) relative.  An f16 output adds one rounding to nearest: 2^-11 relative, or half the smallest subnormal step, 2^-25.
"""
import numpy as np

from index_reference import TOL, U, gamma


# ------------------------------------------------------------------------------------------------
# MaxSim
# ------------------------------------------------------------------------------------------------
def round_f16(rows):
    """what the host form scores: the f32 rows rounded to f16 (nearest even), as float64"""
    return np.asarray(rows, dtype=np.float32).astype(np.float16).astype(np.float64)


def pair_reference(q, d, mean=False):
    """q [nq, H], d [nd, H] float64 (f16 values) -> (score, bound) of one pair"""
    S = q @ d.T
    tol = TOL * (np.abs(q) @ np.abs(d).T)
    M, t = S.max(axis=1), tol.max(axis=1)
    n = len(q)
    score, bound = float(M.sum()), float(t.sum() + gamma(n) * (np.abs(M) + t).sum())
    if mean:
        score, bound = score / n, bound / n
        bound += U * (abs(score) + bound)
    return score, bound


def maxsim_reference(q, qcu, d, dcu, pairs=None, mean=False):
    """(scores, bounds) float64, [n_q, n_d] or [n_pairs]; q, d: the rows as the kernel reads them (f16 values)"""
    q, d = np.asarray(q, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n_q, n_d = len(qcu) - 1, len(dcu) - 1
    todo = [(a, b) for a in range(n_q) for b in range(n_d)] if pairs is None else [tuple(p) for p in np.asarray(pairs).reshape(-1, 2)]
    out = np.array([pair_reference(q[qcu[a]:qcu[a + 1]], d[dcu[b]:dcu[b + 1]], mean) for a, b in todo])
    s, bd = out[:, 0], out[:, 1]
    return (s.reshape(n_q, n_d), bd.reshape(n_q, n_d)) if pairs is None else (s, bd)


def chain_f32(q, d):
    """[nq, nd] float32: the inner products restated in NumPy f32 arithmetic — k ascending in steps of 16 (a short last step at
    H % 16 == 8), the 16 products of a step added in f32, the steps accumulated in f32"""
    q, d = np.asarray(q, dtype=np.float32), np.asarray(d, dtype=np.float32)
    acc = np.zeros((len(q), len(d)), dtype=np.float32)
    for k in range(0, q.shape[1], 16):
        step = np.zeros_like(acc)
        for e in range(k, min(k + 16, q.shape[1])):
            step = step + np.outer(q[:, e], d[:, e]).astype(np.float32)
        acc = acc + step
    return acc


def maxsim_f32(q, qcu, d, dcu, pairs=None, mean=False):
    """the score restated in NumPy f32: chain_f32, an exact max, the query tokens' maxima added one after the other in f32"""
    n_q, n_d = len(qcu) - 1, len(dcu) - 1
    todo = [(a, b) for a in range(n_q) for b in range(n_d)] if pairs is None else [tuple(p) for p in np.asarray(pairs).reshape(-1, 2)]
    out = np.empty(len(todo), dtype=np.float32)
    for i, (a, b) in enumerate(todo):
        M = chain_f32(q[qcu[a]:qcu[a + 1]], d[dcu[b]:dcu[b + 1]]).max(axis=1)
        s = np.float32(0)
        for v in M:
            s = np.float32(s + v)
        out[i] = np.float32(s / np.float32(len(M))) if mean else s
    return out.reshape(n_q, n_d) if pairs is None else out


def unit_rows(rng, n, H):
    x = rng.normal(0, 1, (n, H))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def packed_set(rng, lens, H, front=0, behind=0, junk_every=0, rows=None):
    """A packed set of sentences of these lengths: (rows f32 [., H], cu int32, real) — `front` NaN rows in front of the first sentence
    (cu[0] = front), `behind` NaN rows behind the last, and, with junk_every = j, a sentence of three NaN rows after every j-th real
    one: `real` lists the indices of the real sentences, the only ones a pair list may name.  rows(n): the real rows' maker."""
    make = rows if rows is not None else (lambda n: unit_rows(rng, n, H))
    parts, cu, real = [np.full((front, H), np.nan, np.float32)], [front], []
    for i, n in enumerate(lens):
        real.append(len(cu) - 1)
        parts.append(make(n)); cu.append(cu[-1] + n)
        if junk_every and (i + 1) % junk_every == 0:
            parts.append(np.full((3, H), np.nan, np.float32)); cu.append(cu[-1] + 3)
    parts.append(np.full((behind, H), np.nan, np.float32))
    return np.concatenate(parts).astype(np.float32), np.asarray(cu, dtype=np.int32), real


def negative_sets(rng, qlens, dlens, H):
    """Queries near one unit vector, documents near its negative: every true similarity is about -1.  (q rows, qcu, d rows, dcu)"""
    base = unit_rows(rng, 1, H)[0]
    near = lambda sign: (lambda n: (sign * base + 0.05 * unit_rows(rng, n, H)).astype(np.float32))
    q, qcu, _ = packed_set(rng, qlens, H, rows=near(1.0))
    d, dcu, _ = packed_set(rng, dlens, H, rows=near(-1.0))
    return q, qcu, d, dcu


# ------------------------------------------------------------------------------------------------
# token rows
# ------------------------------------------------------------------------------------------------
def token_rows_reference(x, normalize, f16_out):
    """x [T, H] stored states (f16 or f32) -> (rows float64, bound float64)"""
    x64 = np.asarray(x).astype(np.float64)
    H = x64.shape[1]
    want = x64 / np.sqrt((x64 * x64).sum(axis=1, keepdims=True)) if normalize else x64
    bound = gamma(H + 2) * np.abs(want) if normalize else np.zeros_like(want)
    if f16_out:
        bound = bound + np.maximum(2.0 ** -11 * (np.abs(want) + bound), 2.0 ** -25)
    return want, bound
