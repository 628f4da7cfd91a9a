"""NumPy restatement of the mxfp4 index's two stored forms (include/bert_hip.h), float64 inside: rows as OCP MXFP4 (e2m1 codes),
queries as MXFP8 (e4m3 codes), one power-of-two scale per block of 32 elements.  Both return the decoded values as float32
[n, dim], which is what bert_hip_index_get_rows returns for rows; a row or query with a NaN or an inf comes back all NaN."""
import numpy as np


def _mx(x, emax, mant, emin, vmax):
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    bad = ~np.isfinite(x).all(axis=1)
    dpad = (dim + 63) // 64 * 64
    b = np.zeros((n, dpad))
    b[:, :dim] = np.where(bad[:, None], 0, x)
    b = b.reshape(n, dpad // 32, 32)
    amax = np.abs(b).max(axis=2)
    e = np.where(amax == 0, 0, np.clip(np.frexp(amax)[1] - 1 - emax, -127, 127))[:, :, None]      # frexp - 1 = floor(log2)
    y = np.ldexp(b, -e)                                              # exact
    ex = np.maximum(np.frexp(np.abs(y))[1] - 1, emin)                # the binade, from the subnormals' up
    q = np.minimum(np.ldexp(np.rint(np.ldexp(np.abs(y), mant - ex)), ex - mant), vmax)             # rint: ties to even
    out = np.ldexp(np.copysign(q, y), e).reshape(n, dpad)[:, :dim].astype(np.float32)                # exact in float32
    out[bad] = np.nan
    return out


def mxfp4_rows(x):
    """e2m1: grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, e = floor(log2(amax)) - 2"""
    return _mx(x, 2, 1, 0, 6.0)


def mxfp8_queries(x):
    """e4m3: bias 7, subnormals (least normal 2^-6), largest 448, e = floor(log2(amax)) - 8"""
    return _mx(x, 8, 3, -6, 448.0)
