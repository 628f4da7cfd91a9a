"""Float64 reference, derived bound and the float32 restatement of the norm's order for csrc/token_proj.hip.  No GPU.

out[t] = Wp x[t] over the f16 operands in float64, then, normalised, over its own L2 norm.  The bound per value v = out[t][p]:
  - the f16 MFMA chain over H products with f32 accumulation: maxsim_reference.py's per-dot bound, e = TOL * sum_k |Wp[p][k] x[t][k]|;
  - un-normalised, the f32 output is that value: bound e;
  - normalised: with n = ||v||_2 and E = ||e||_2 over the row, the computed row's true norm n' lies in [n - E, n + E]; the scale is 1 / n'
    up to P rounded squares, P - 1 additions, a correctly rounded sqrt (which halves the error) and reciprocal, and with the final
    multiplication gamma(P + 2) relative (token_rows_reference's count):
        |got - v / n| <= |v| E / (n (n - E)) + e / (n - E) + gamma(P + 2) (|v| + e) / (n - E),   infinite where E >= n;
  - an f16 output adds one rounding to nearest: 2^-11 relative, or half the smallest subnormal step, 2^-25.
"""
import numpy as np

from index_reference import TOL, gamma

def project_reference(x, wp, normalize, f16_out):
    """x [T, H], wp [P, H] float16 -> (rows float64 [T, P], bound float64)"""
    x64, w64 = np.asarray(x).astype(np.float64), np.asarray(wp).astype(np.float64)
    v, e = x64 @ w64.T, TOL * (np.abs(x64) @ np.abs(w64).T)
    want, bound = v, e
    if normalize:
        P = w64.shape[0]
        n, E = np.sqrt((v * v).sum(axis=1, keepdims=True)), np.sqrt((e * e).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            want = v / n
            bound = np.where(E < n, (np.abs(v) * E / n + e + gamma(P + 2) * (np.abs(v) + e)) / (n - E), np.inf)
    if f16_out:
        bound = bound + np.maximum(2.0 ** -11 * (np.abs(want) + bound), 2.0 ** -25)
    return want, bound

def normalize_f32(v):
    """The kernel's norm in NumPy float32 on f32 rows v [T, P]: a lane holds the features f with (f % 8) // 4 == h and adds their
    squares — each rounded — in ascending order; the h = 0 sum plus the h = 1 sum; 1 / sqrt; value * scale."""
    v = np.asarray(v, dtype=np.float32)
    s = np.zeros((2, len(v)), dtype=np.float32)
    for f in range(v.shape[1]):
        s[(f % 8) // 4] = s[(f % 8) // 4] + v[:, f] * v[:, f]
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.float32(1) / np.sqrt(s[0] + s[1])
        return v * scale[:, None]

def exact_operands(rng, T, H, P):
    """Small integers as f16: every product and every partial sum of the chain is exact in f32, whatever the order"""
    return rng.integers(-4, 5, (T, H)).astype(np.float16), rng.integers(-3, 4, (P, H)).astype(np.float16)
