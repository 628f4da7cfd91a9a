"""The sparse index's contract in plain Python / NumPy (include/bert_hip.h "Sparse index"): the score rule with every fmaf step rounded
ONCE to f32, the order rule, and the stored form of a row.  No GPU, no library.

The score of a (query, row) pair is   acc = +0; for each stored term (id, w) of the row in ascending id that the query has:
acc = fmaf(w, q[id], acc)   in f32.  fma_f32 computes one step from the exact rational w * q + acc (fractions) and rounds it to the nearest
even f32 — never through a float64 sum, which can round twice.  scores() is the same rule over whole arrays: it uses float64 only where
that is provably the same single rounding (see _fma_f32_array) and falls back to fma_f32 elsewhere."""
from fractions import Fraction
import math

import numpy as np

_TWO = Fraction(2)


def round_f32(x: Fraction) -> np.float32:
    """The f32 nearest to the exact rational x, ties to even; +0 for 0; +-inf beyond the range (IEEE overflow)."""
    if x == 0:
        return np.float32(0.0)
    neg, a = x < 0, abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < _TWO ** e:
        e -= 1                                   # 2^e <= a < 2^(e + 1)
    e = max(e, -126)                             # below: the subnormals' spacing
    q = a / _TWO ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    v = Fraction(n) * _TWO ** (e - 23)
    if v >= _TWO ** 128:
        f = math.inf
    else:
        f = float(v)                             # exact: at most 25 significant bits, an exponent a double holds
    return np.float32(-f if neg else f)


def fma_f32(w, q, acc) -> np.float32:
    """fmaf(w, q, acc) for finite f32 operands: the exact w * q + acc rounded once."""
    w, q, acc = float(np.float32(w)), float(np.float32(q)), float(np.float32(acc))
    exact = Fraction(w) * Fraction(q) + Fraction(acc)
    if exact != 0:
        r = round_f32(exact)
        # (a non-zero exact result that underflows keeps its sign)
        return np.float32(math.copysign(float(r), -1.0 if exact < 0 else 1.0))
    # an exact zero: IEEE's sum of zeros (equal signs keep it, else +0); an exact cancellation of non-zero operands is +0
    if w * q == 0 and acc == 0:
        ps = math.copysign(1.0, w) * math.copysign(1.0, q)
        return np.float32(-0.0 if (ps < 0 and math.copysign(1.0, acc) < 0) else 0.0)
    return np.float32(0.0)


def score(row_ids, row_w, q_ids, q_w) -> np.float32:
    """One (query, row) score, scalar: row_ids ascending then -1 (a stored row), the query in any order with -1 for unused places."""
    q = {int(i): np.float32(w) for i, w in zip(q_ids, q_w) if i >= 0}
    acc = np.float32(0.0)
    for i, w in zip(row_ids, row_w):
        if i >= 0 and int(i) in q:
            acc = fma_f32(w, q[int(i)], acc)
    return acc


def _fma_f32_array(w, q, acc):
    """fma_f32 over float32 arrays.  p = w * q is exact in float64 (48 significant bits); s = p + acc is the float64 nearest to the
    exact sum.  Rounding s to f32 equals rounding the exact sum unless the float64 add was inexact AND s sits exactly half-way between two
    f32 (its low 29 mantissa bits are 1 0...0): only then could the second rounding go the other way.  Those elements, and results
    near the subnormal range (where the half-way pattern differs), go through fma_f32."""
    w64, q64, a64 = w.astype(np.float64), q.astype(np.float64), acc.astype(np.float64)
    p = w64 * q64
    s = p + a64
    bb = s - a64
    err = (a64 - (s - bb)) + (p - bb)            # TwoSum: zero iff the add was exact
    low = s.view(np.uint64) & np.uint64((1 << 29) - 1)
    tiny = (np.abs(s) < 2.0 ** -125) & (s != 0)
    redo = ((err != 0) & (low == np.uint64(1 << 28))) | tiny
    with np.errstate(over="ignore"):
        out = s.astype(np.float32)
    for i in np.flatnonzero(redo):
        out.flat[i] = fma_f32(w.flat[i], q.flat[i], acc.flat[i])
    return out


def scores(st_ids, st_w, q_ids, q_w, n_vocab):
    """All scores [nq][n_rows] f32: stored rows (st_ids / st_w [n][width] as stored_rows returns them) against queries [nq][kq]."""
    st_ids, st_w = np.asarray(st_ids, np.int32), np.asarray(st_w, np.float32)
    q_ids, q_w = np.asarray(q_ids, np.int32), np.asarray(q_w, np.float32)
    n, width = st_ids.shape
    out = np.zeros((q_ids.shape[0], n), np.float32)
    for qi in range(q_ids.shape[0]):
        dense = np.zeros(n_vocab, np.float32)
        has = np.zeros(n_vocab, bool)
        ok = q_ids[qi] >= 0
        dense[q_ids[qi][ok]] = q_w[qi][ok]
        has[q_ids[qi][ok]] = True
        acc = np.zeros(n, np.float32)
        for j in range(width):
            idj = st_ids[:, j]
            hit = idj >= 0
            hit[hit] = has[idj[hit]]
            if hit.any():
                acc[hit] = _fma_f32_array(st_w[hit, j], dense[idj[hit]], acc[hit])
        out[qi] = acc
    return out


def topk(row_scores, k):
    """The order rule over one query's scores [n_rows]: larger score first, equal scores (==) smaller id first, NaN never returned,
    missing entries id -1 / score -inf.  Returns (ids [k] int32, scores [k] f32)."""
    s = np.asarray(row_scores, np.float32)
    ids = np.flatnonzero(~np.isnan(s))
    order = ids[np.lexsort((ids, -s[ids].astype(np.float64)))][:k]
    out_i = np.full(k, -1, np.int32)
    out_s = np.full(k, -np.inf, np.float32)
    out_i[:len(order)] = order
    out_s[:len(order)] = s[order]
    return out_i, out_s


def search(st_ids, st_w, q_ids, q_w, n_vocab, k):
    """(ids [nq][k], scores [nq][k]) of an exact search."""
    sc = scores(st_ids, st_w, q_ids, q_w, n_vocab)
    res = [topk(r, k) for r in sc]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def stored_rows(ids, weights, width, dtype):
    """The stored form of rows ids / weights [n][k_in] (ids in [-1, n_vocab), none twice): per row the used places sorted by id, the
    weights as stored (dtype "f16": rounded to nearest even f16, returned as the exact f32), then id -1 with weight +0 up to width."""
    ids, weights = np.asarray(ids, np.int32), np.asarray(weights, np.float32)
    n = ids.shape[0]
    out_i = np.full((n, width), -1, np.int32)
    out_w = np.zeros((n, width), np.float32)
    for r in range(n):
        used = ids[r] >= 0
        order = np.argsort(ids[r][used], kind="stable")
        w = weights[r][used][order]
        if dtype == "f16":
            with np.errstate(over="ignore"):
                w = w.astype(np.float16).astype(np.float32)
        out_i[r, :len(order)] = ids[r][used][order]
        out_w[r, :len(order)] = w
    return out_i, out_w
