"""References for the token index's int8 form (include/bert_hip.h "TOKEN INDEX, int8 form"; tests: test_late_i8_host.py,
test_gpu_late_i8.py).  No GPU.  Written from the header's text, not from the kernel.

quantise.  Per row, in float32: scale = amax / 127; code_i = clamp(rint(x_i / scale), -127, 127) (NumPy's float32 division is the
correctly rounded IEEE one, rint rounds to nearest even); all codes 0 where the scale is 0; scale NaN and codes 0 where an element is
NaN or +-inf.  Codes are padded with zeros to dpad, dim rounded up to a multiple of 32.

scores_i8.  Every step of the score is exact or one correctly rounded float32 operation in a stated order, so NumPy float32 gives its
bits: dot_ij as an integer (computed by a float32 matrix product, which is exact here: every partial sum is an integer of magnitude at
most 1024 x 127^2 < 2^24, whatever the order), m_i = max_j (float32(dot_ij) * ds_j), t_i = m_i * qs_i, the t_i of a block of 32 query
tokens added in the butterfly order of wave_sum (lane ^ 32 first — the upper half of the wave holds +0 —, then ^ 16, 8, 4, 2, 1; +0 in
the slots behind the query's end), the blocks' sums added in ascending order from +0.  A document with a NaN scale scores NaN, and so
does every document for a query with one.

scores_f64.  The float64 MaxSim of the UNQUANTISED rows, sum_i max_j <q_i, d_j>, and a bound on |scores_i8 - it| derived here:
  - an element x of a row with scale s is stored as c with |x - c s| <= s (1/2 + 127 u), u = 2^-24: rint is within 1/2 of the float32
    quotient, the quotient within u |x / s| <= 127 (1 + 2u) u of the real one, and the clamp moves nothing that lies beyond 127 by more
    than that (|x| <= amax, s >= (amax / 127)(1 - u)); written h(s) = s (1/2 + 2^-17) below;
  - so for the dequantised rows qhat_i, dhat_j:  |<q_i, d_j> - <qhat_i, dhat_j>| <= h(qs_i) ||d_j||_1 + h(ds_j) ||qhat_i||_1
    (<q - qhat, d> + <qhat, d - dhat>);
  - the kernel's product float32(dot) * ds_j * qs_i is <qhat_i, dhat_j> under two float32 roundings: within (2u + u^2) |<qhat_i, dhat_j>|;
    qs_i >= 0 and rounding is monotone, so multiplying behind the max is multiplying in front of it;
  - the max is exact and monotone: token i's maximum is off by at most t_i = max_j of the two terms above;
  - the float32 sum over the n query tokens passes a value through at most n - 1 roundings (adding +0 is exact):
    gamma(n) * sum_i (|M_i| + t_i) with the float64 maxima M_i, as maxsim_reference.pair_reference has it.
No underflow occurs at the magnitudes the tests use (rows of norm 1 .. 6e4)."""
import numpy as np

from index_reference import U, gamma


def dpad(dim):
    return (dim + 31) // 32 * 32


def quantise(rows):
    """rows [n, dim] -> (codes int8 [n, dpad], scales float32 [n])"""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = x.shape
    codes = np.zeros((n, dpad(dim)), np.int8)
    scales = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for r in range(n):
            if not np.isfinite(x[r]).all():
                scales[r] = np.nan
                continue
            scale = np.float32(np.abs(x[r]).max()) / np.float32(127.0)
            scales[r] = scale
            if scale == 0:
                continue
            codes[r, :dim] = np.clip(np.rint(x[r] / scale), -127.0, 127.0).astype(np.int8)
    return codes, scales


def butterfly_sum(v):
    """v float32 [32, ...]: what lane 0 of wave_sum holds for a wave whose lanes 0 .. 31 hold v and whose lanes 32 .. 63 hold +0"""
    v = np.asarray(v, dtype=np.float32) + np.float32(0)                      # (lane ^ 32)
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    return v[0]


def _token_products(qc, qs, dc, ds, dcu):
    """m [n_q_tokens, n_docs] float32: max over a document's tokens of float32(dot) * ds"""
    dots = qc.astype(np.float32) @ dc.astype(np.float32).T                   # exact integers (the module's text)
    with np.errstate(invalid="ignore"):
        p = dots * ds[None, :]
    return np.maximum.reduceat(p, np.asarray(dcu[:-1], dtype=np.int64), axis=1)


def scores_i8(q, qcu, d, dcu):
    """[n_queries, n_docs] float32, the bits an int8 index gives; NaN where the document or the query holds a non-finite token"""
    qc, qs = quantise(q[qcu[0]:qcu[-1]])
    dc, ds = quantise(d[dcu[0]:dcu[-1]])
    qcu, dcu = np.asarray(qcu, np.int64) - qcu[0], np.asarray(dcu, np.int64) - dcu[0]
    n_d = len(dcu) - 1
    bad_doc = np.logical_or.reduceat(np.isnan(ds), dcu[:-1]) if n_d else np.zeros(0, bool)
    out = np.empty((len(qcu) - 1, n_d), np.float32)
    with np.errstate(invalid="ignore"):
        for a in range(len(qcu) - 1):
            sl = slice(qcu[a], qcu[a + 1])
            if np.isnan(qs[sl]).any() or n_d == 0:
                out[a] = np.nan
                continue
            t = _token_products(qc[sl], qs[sl], dc, ds, dcu) * qs[sl, None]
            n = len(t)
            t = np.concatenate([t, np.zeros(((-n) % 32, n_d), np.float32)])
            total = np.zeros(n_d, np.float32)
            for b in range(0, len(t), 32):
                total = total + butterfly_sum(t[b:b + 32])
            out[a] = total
    out[:, bad_doc] = np.nan
    return out


def scores_f64(q, qcu, d, dcu):
    """(scores, bounds) float64 [n_queries, n_docs]: the MaxSim of the unquantised rows and the bound of the module's text (finite rows)"""
    q64, d64 = np.asarray(q, np.float64), np.asarray(d, np.float64)
    qc, qs = quantise(q)
    dc, ds = quantise(d)
    dim = q64.shape[1]
    qhat, dhat = qc[:, :dim].astype(np.float64) * qs[:, None].astype(np.float64), dc[:, :dim].astype(np.float64) * ds[:, None].astype(np.float64)
    h = lambda s: s.astype(np.float64) * (0.5 + 2.0 ** -17)
    starts = np.asarray(dcu[:-1], dtype=np.int64)
    n_q, n_d = len(qcu) - 1, len(dcu) - 1
    S, B = np.empty((n_q, n_d)), np.empty((n_q, n_d))
    d_l1 = np.abs(d64).sum(axis=1)
    for a in range(n_q):
        sl = slice(qcu[a], qcu[a + 1])
        P = q64[sl] @ d64.T
        tol = h(qs[sl])[:, None] * d_l1[None, :] + np.abs(qhat[sl]).sum(axis=1)[:, None] * h(ds)[None, :]
        tol = tol + (2 * U + U * U) * np.abs(qhat[sl] @ dhat.T)
        M = np.maximum.reduceat(P[:, dcu[0]:dcu[-1]], starts - dcu[0], axis=1)
        t = np.maximum.reduceat(tol[:, dcu[0]:dcu[-1]], starts - dcu[0], axis=1)
        n = qcu[a + 1] - qcu[a]
        S[a] = M.sum(axis=0)
        B[a] = t.sum(axis=0) + gamma(n) * (np.abs(M) + t).sum(axis=0)
    return S, B
