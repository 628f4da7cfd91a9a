"""Float64 restatement of everything of an encoder layer behind the attention (reference bert.cpp:859-901), shared by the tests of
the one-launch layer tail (test_gpu_parity.py) and of the latency route's kernels (test_gpu_latency_kernels.py); and, for the
value-range tests (test_gpu_value_ranges.py on the GPU, test_value_bounds_host.py without one): per-element error bounds derived from
the roundings the kernels perform, NumPy emulations of the device arithmetic those bounds are about, and the inputs both files use."""
import numpy as np

U16 = 2.0 ** -11          # unit roundoff of f16 (round to nearest): |fl(a) - a| <= U16 |a|
U32 = 2.0 ** -24          # of f32
LN2 = float(np.log(2.0))


def f8(a):
    return np.asarray(a).astype(np.float64)


def ulp16(a):
    """the spacing of f16 at |a| (2^-24 in the subnormals): what one rounding to f16 can cost, and twice that"""
    with np.errstate(over="ignore"):
        return f8(np.spacing(np.minimum(np.abs(f8(a)), 65504.0).astype(np.float16)))


def layernorm(v, g, b):
    mu = v.mean(axis=1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True)
    return (v - mu) / np.sqrt(var + 1e-5) * g + b


def gelu(u):
    return 0.5 * u * (1 + np.tanh(0.7978845608028654 * u * (1 + 0.044715 * u * u)))


def layer_tail(ctx, x, Wo, W1, W2, bo, g1, be1, b1, b2, g2, be2):
    """y = LayerNorm(ctx Wo^T + bo + x), out = LayerNorm(gelu(y W1^T + b1) W2^T + b2 + y), with the two roundings to f16 the device
    makes on the way: y (mat-mul input and residual) and the GELU'ed intermediate."""
    y = layernorm(f8(ctx) @ f8(Wo).T + bo + f8(x), g1, be1)
    y16 = f8(y.astype(np.float16))                       # the device keeps y in f16 (GEMM input and residual)
    gl = gelu(y16 @ f8(W1).T + b1)
    return layernorm(f8(gl.astype(np.float16)) @ f8(W2).T + b2 + y16, g2, be2)


# ------------------------------------------------------------------------------------------------
# derived bounds
# ------------------------------------------------------------------------------------------------
def matmul_bound(A, W, bias, resid):
    """f32 accumulation of exact f16 products, K + 2 terms in any order: (K + 4) 2^-24 S to first order, S the sum of the terms'
    magnitudes; times 4 for the matrix cores' undocumented internal rounding."""
    S = np.abs(f8(A)) @ np.abs(f8(W)).T + np.abs(f8(bias)) + np.abs(f8(resid))
    return 4 * (A.shape[1] + 4) * U32 * S, S


def layernorm_stats_bound(v, one_pass=False):
    """(|mean error|, |error of 1 / std| / (1 / std)) of f32 row statistics, to first order: a sum of H terms in any order is off by
    at most H 2^-24 sum |v|, so the mean by H 2^-24 mean |v|, and 1 / std by that fraction of itself; twice both for the squares'
    sum and the arithmetic behind.
    one_pass: the variance is E[v^2] - mean^2 (device.h layernorm_scale, ln_rows_finalize), not the mean of (v - mean)^2.  The sum
    of squares is off by at most H 2^-24 E[v^2] and mean^2 by 2 |mean| times the mean's error, H 2^-24 mean |v|; twice both as
    above.  That ABSOLUTE error of the variance, 2 H 2^-24 (E[v^2] + 2 |mean| mean |v|), is a fraction
    2 H 2^-24 (var + mean^2 + 2 |mean| mean |v|) / var of it -- about 2 H 2^-24 (1 + 3 (mean / std)^2) -- and half that fraction
    of 1 / std and of every normalised value."""
    v = f8(v)
    H = v.shape[1]
    mu = v.mean(axis=1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5
    mean_abs = np.abs(v).mean(axis=1, keepdims=True)
    rstd_rel = 2 * H * U32 * np.ones_like(mu)
    if one_pass:
        rstd_rel = rstd_rel + H * U32 * ((v * v).mean(axis=1, keepdims=True) + 2 * np.abs(mu) * mean_abs) / var
    return 2 * H * U32 * mean_abs, rstd_rel


def layernorm_bound(v, g, want, one_pass=False, rounding=None):
    """One f16 ulp of the value for the rounding, and the f32 statistics (layernorm_stats_bound): the mean's error is an ABSOLUTE
    error of every v - mean, which a value that beta all but cancels does not scale down.  (A bound relative to the value alone is
    not one: with 768 x 384 draws a value of 6e-5 beside a beta of -0.016 comes out 1.1 subnormal ulp away.)
    rounding: what the roundings of the output cost instead, for a kernel that does not store f16 (f32_reference.layernorm_bound)."""
    v = f8(v)
    mu = v.mean(axis=1, keepdims=True)
    sd = np.sqrt(((v - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5)
    mean_err, rstd_rel = layernorm_stats_bound(v, one_pass)
    return (ulp16(want) if rounding is None else rounding) + (mean_err + np.abs(v - mu) * rstd_rel) / sd * np.abs(f8(g))


def layernorm_input_term(v, g, dv):
    """What errors of at most dv (per element) in the rows v cost LayerNorm(v) g, to first order: the element's own error and the
    mean's, over std, and the fraction rms(dv) / std of every normalised value (the change of std is at most rms(dv))"""
    v, dv = f8(v), np.broadcast_to(f8(dv), np.shape(v))
    mu = v.mean(axis=1, keepdims=True)
    sd = np.sqrt(((v - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5)
    rms = np.sqrt((dv * dv).mean(axis=1, keepdims=True))
    return (dv + dv.mean(axis=1, keepdims=True) + np.abs(v - mu) / sd * rms) / sd * np.abs(f8(g))


def one_pass_limit(H):
    """mean / std at which layernorm_bound's one-pass term reaches one f16 ulp (2^-10) of a normalised value of magnitude 1:
    H 2^-24 (1 + 3 r^2) = 2^-10"""
    return float(np.sqrt((2.0 ** 14 / H - 1) / 3))


_C1 = -2.0 * 0.79788456080286535588 * 1.44269504088896340736        # gelu(x) = x / (1 + 2^t), t = x (C1 + C2 x^2)
_C2 = _C1 * 0.044715
GELU_FLUSH = 2.0 ** -14


def gelu_bound(pre):
    """|device - gelu(pre)| for gelu_pk16h (device.h) on the f32 pre-activation `pre`, per element:
      - the pre-activation is rounded to f16 first: |gelu(x) - gelu(pre)|, x = f16(pre), exactly;
      - t = x (C1 + C2 x^2) in f16: x x, the multiply-add and the product with x round once each, a fourth time if the compiler does
        not fuse the multiply-add, and C1, C2 are themselves f16 (both negative: no cancellation): |dt| <= 5 U16 |t|.  With
        E = 2^t and s = E / (1 + E), dt changes 1 / (1 + E) by the fraction s ln 2 |dt| of itself;
      - v_exp_f16: one ulp (2^-10) of E, the fraction s of that in 1 / (1 + E); 1 + E rounds once (U16); v_rcp_f16: one ulp, or
        2^-24 (1 + E) once the reciprocal is a subnormal;
      - the product with x rounds once: one f16 ulp of the result (2^-24 for a subnormal one);
      - where the device's t may reach 16, 2^t is infinite in f16 and the result is -0: the one absolute term, GELU_FLUSH."""
    pre = f8(pre)
    x = f8(pre.astype(np.float16))
    gx = gelu(x)
    t = x * (_C1 + _C2 * x * x)
    E = np.exp2(np.minimum(t, 40.0))
    s = E / (1 + E)
    rel = s * (LN2 * 5 * U16 * np.minimum(np.abs(t), 40.0) + 2.0 ** -10) + U16 + np.maximum(2.0 ** -10, U32 * (1 + E))
    bound = np.abs(gx - gelu(pre)) + rel * np.abs(gx) + ulp16(gx)
    return bound + np.where(t * (1 + 5 * U16) >= 16, GELU_FLUSH, 0.0)


def gelu_rounds_to_x(pre):
    """where float64 gelu(x) of the f16 pre-activation x = f16(pre) rounds to x itself (large positive values, and the zeros):
    there the device must return exactly x.  Not asked of subnormal values: gelu(x) is a hair more than x / 2 there, which can round
    to x where the device's x times an exact 0.5 is a tie."""
    x = f8(pre).astype(np.float16)
    return (gelu(f8(x)).astype(np.float16) == x) & ((np.abs(f8(x)) >= 2.0 ** -14) | (x == 0))


def softmax_bound(q, k, v, scale):
    """|device - softmax(q k^T scale) v| for one head (q [n][d], k [n][d], v [n][d] f16 values), per element, to first order, for
    attention.hip's online softmax (device.h softmax_p8): with p_j = exp(score_j - max), L = sum p, w = p / L,
      - the scores are f32 sums of exact f16 products (matmul_bound); the argument of exp2 is one fma of the score, the f32 scale
        log2(e) / sqrt(d) (two roundings) and the chunk's running maximum (whose own rounding cancels between the numerators and
        the rescaling factors): 2^-22 |score_j - max|; the rescaling across 128-key chunks subtracts running maxima, which only
        grow: 2^-24 (max - first chunk's max) in all; v_exp_f32 one ulp, doubled, per chunk passed.  Relative to p_j: eps_j;
      - P rounds to f16 for the second mat-mul: U16 p_j, or half a subnormal ulp, 2^-25, of the scale on which the largest p is 1;
      - L is an f32 sum of the un-rounded p, the output an f32 sum of exact products, rescaled per chunk and divided by L:
        (n + 8) 2^-24 of sum w |v| and twice that, times 4 for the matrix cores as in matmul_bound;
      - the result rounds to f16 once: one ulp.
    Weighted by |v|: sum_j (|dw_j|) |v_j| with |dw_j| <= w_j eps_j + max(U16 w_j, 2^-25 / L) + w_j sum_k w_k eps_k."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    sc = q @ k.T * scale
    ds = 4 * (d + 4) * U32 * (np.abs(q) @ np.abs(k).T) * scale            # natural-log units
    mx = sc.max(axis=1, keepdims=True)
    first = sc[:, :128].max(axis=1, keepdims=True)
    n_chunks = (n + 127) // 128
    # (a rounding of the exp2 argument is the same fraction of the argument in base-2 and in natural units)
    eps = ds + 2.0 ** -22 * (mx - sc) + U32 * (mx - first) + (n_chunks + 1) * 2.0 ** -22
    p = np.exp(sc - mx)
    L = p.sum(axis=1, keepdims=True)
    w = p / L
    dw = w * eps + np.maximum(U16 * w, 2.0 ** -25 / L) + w * (w * eps).sum(axis=1, keepdims=True)
    want = w @ v
    wv = w @ np.abs(v)
    return dw @ np.abs(v) + 8 * (n + 8) * U32 * wv + ulp16(want), want


# The generic kernels (gemm_naive_kernel, attention_naive_kernel): one thread an element, plain f32 loops, no matrix cores.
#
# __expf(x) is exp2(x log2(e)) on v_exp_f32.  No run has measured it here (f32_reference.py measured the device's tanhf only and
# takes expf from the OpenCL profile, EXPF_ULP = 3 ulp -- the library function, which this is not); its error is derived:
#   - log2(e) is an f32 constant (u of it) and the product with x rounds once: the argument of exp2 is off by 2 u |x log2(e)|,
#     which exp2 turns into the fraction 2 u |x| of the result;
#   - v_exp_f32 is documented to 1 ulp (2 u of the result); NATIVE_EXP2_ULP allows two;
#   - a result below 2^-126 is flushed to zero: an absolute 2^-126.
NATIVE_EXP2_ULP = 2.0


def native_expf_rel(x):
    """the fraction of exp(x) by which the device's __expf(x) may differ from it (besides the flush below 2^-126)"""
    return 2 * U32 * np.abs(f8(x)) + 2 * NATIVE_EXP2_ULP * U32


def generic_matmul_bound(A, W, bias, resid=None):
    """|gemm_naive_kernel - (A W^T + bias (+ resid))| before the GELU, A and W f16 values, as f32_reference.matmul_bound derives it
    for an f32 chain, plus the rounding of the result to f16:
      - the products of two f16 numbers are exact in f32 (22 bits), fused or not; the accumulator is ONE ascending chain of K f32
        additions: at most g_K S, g_K = K u / (1 - K u), S = sum_k |a_k w_k|;
      - + bias rounds once: u (|A W^T + bias| + g_K S); with a residual one more addition, u |want|;
      - g_K (1 + 2 u) <= (K + 1) u while K^2 u <= 1 (K <= 4096); (K + 2) leaves that room twice.  No factor 4: no matrix cores;
      - the result rounds to f16 once: ulp16(want) (twice what a rounding to nearest costs; the slack covers the rounding boundary
        the f32 error can push the value across).
    Returns (bound, want, pre, dpre): pre = A W^T + bias and the most the device's f32 one differs from it."""
    K = np.shape(A)[1]
    S = np.abs(f8(A)) @ np.abs(f8(W)).T
    pre = f8(A) @ f8(W).T + f8(bias)
    dpre = (K + 2) * U32 * S + U32 * np.abs(pre)
    want = pre if resid is None else pre + f8(resid)
    return dpre + (0 if resid is None else U32 * np.abs(want)) + ulp16(want), want, pre, dpre


def generic_gemm_bound(A, W, bias, resid, epilogue):
    """(bound, want) of one call of gemm_naive_kernel under `epilogue` (0 bias, 1 bias + GELU, 2 bias + resid).  GELU: gelu_tanh
    (gemm.hip) evaluates x / (1 + exp2(t)) in f32; gelu_bound is derived for the same formula evaluated in f16 on the f16-rounded
    pre-activation and admits every f32 evaluation of it (test_gpu_value_ranges.py holds this kernel to it), and |gelu'| <= 1.13
    carries the pre-activation's own error."""
    bound, want, pre, dpre = generic_matmul_bound(A, W, bias, resid if epilogue == 2 else None)
    if epilogue == 1:
        return gelu_bound(pre) + 1.13 * dpre, gelu(pre)
    return bound, want


def generic_attention_bound(q, k, v):
    """|attention_naive_kernel - softmax(q k^T / sqrt(d)) v| for one head (q, k, v [n][d] f16 values), per element, to first order:
    a two-pass softmax (the TRUE maximum is subtracted, one division at the end), as f32_reference.softmax_bound derives it, with
    p_j = exp(s_j - max), L = sum p, w = p / L:
      - s_j = (sum_e k_e q_e) scale: exact products, a chain of d f32 additions, d u sum |k q|; scale = 1 / sqrtf(d), two roundings,
        and the product a third: (d + 3) u (|q| . |k_j|) scale;
      - s_j - max rounds once, u |s_j - max|; the maximum's own error multiplies every p by the same factor and cancels in p / L;
        __expf: native_expf_rel(s_j - max) of p_j, and the flush: 2^-126 on the scale where the largest p is 1;
      - L is a sum of the n numbers p_j (64 lane chains, then the wave's tree: at most n u), 1 / L rounds once; the output is a chain
        of n terms v_j p_j, each product rounding once unless it is fused, and its product with 1 / L rounds once: (3 n + 2) u sum w |v|;
      - the result rounds to f16 once: ulp16(want).
    |dw_j| <= w_j eps_j + 2^-126 / L + w_j sum_k (w_k eps_k + 2^-126 / L).  Returns (bound, want)."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    scale = 1 / np.sqrt(d)
    sc = q @ k.T * scale
    mx = sc.max(axis=1, keepdims=True)
    eps = (d + 3) * U32 * (np.abs(q) @ np.abs(k).T) * scale + U32 * (mx - sc) + native_expf_rel(sc - mx)
    p = np.exp(sc - mx)
    L = p.sum(axis=1, keepdims=True)
    w = p / L
    dw = w * eps + 2.0 ** -126 / L
    dw = dw + w * dw.sum(axis=1, keepdims=True)
    want = w @ v
    return dw @ np.abs(v) + (3 * n + 2) * U32 * (w @ np.abs(v)) + ulp16(want), want


def generic_attention_packed(qkv, lens, n_head, d_head):
    """qkv [T][3H] f16 of packed sentences -> (float64 context rows [T][H], their bounds)"""
    H = n_head * d_head
    want, bnd = np.zeros((len(qkv), H)), np.zeros((len(qkv), H))
    t0 = 0
    for n in lens:
        for h in range(n_head):
            sl = slice(h * d_head, (h + 1) * d_head)
            q, k, v = (qkv[t0:t0 + n, i * H:(i + 1) * H][:, sl] for i in range(3))
            bnd[t0:t0 + n, sl], want[t0:t0 + n, sl] = generic_attention_bound(q, k, v)
        t0 += n
    return want, bnd


# ------------------------------------------------------------------------------------------------
# NumPy emulations of the device arithmetic the bounds are about
# ------------------------------------------------------------------------------------------------
def gelu_pk16h(x):
    """device.h gelu_pk16h in float16: every operation rounds where the device's does (the multiply-add once); exp2 and the
    reciprocal correctly rounded where the device is within one ulp"""
    x = np.asarray(x).astype(np.float16)
    c1 = np.float32(-2.0) * np.float32(0.79788456080286535588) * np.float32(1.44269504088896340736)
    C1, C2 = np.float16(c1), np.float16(c1 * np.float32(0.044715))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        xx = x * x
        w = (f8(xx) * f8(C2) + f8(C1)).astype(np.float16)
        t = w * x
        e = np.exp2(f8(t)).astype(np.float16)
        d = e + np.float16(1)
        r = (1.0 / f8(d)).astype(np.float16)
        return x * r


def layernorm_one_pass(v, g, b):
    """device.h layernorm_scale on float32 sums of v and v^2 (pairwise, NumPy's order), the output as layernorm_runs_of forms it"""
    v = np.asarray(v, dtype=np.float32)
    g, b = np.asarray(g, dtype=np.float32), np.asarray(b, dtype=np.float32)
    inv_h = np.float32(1.0 / v.shape[1])
    mean = v.sum(axis=1, keepdims=True, dtype=np.float32) * inv_h
    ex2 = (v * v).sum(axis=1, keepdims=True, dtype=np.float32) * inv_h
    t = np.maximum((f8(ex2) - f8(mean) * f8(mean)).astype(np.float32), np.float32(0)) + np.float32(1e-5)       # (one fma)
    rstd = (1.0 / np.sqrt(f8(t))).astype(np.float32)
    nmr = -mean * rstd
    return (v * (g * rstd) + (g * nmr + b)).astype(np.float16)


def softmax_online(q, k, v, scale, chunk=128):
    """attention.hip's online softmax for one head in float32: exp2 of an fma with the f32 scale and the running maximum, the row sum
    of the un-rounded numerators, P rounded to f16, f32 accumulation, the rescale by alpha, the division, one rounding to f16"""
    q, k, v = (np.asarray(a).astype(np.float16) for a in (q, k, v))
    n, d = q.shape
    sc = np.float32(1.44269504088896340736) / np.sqrt(np.float32(1.0 / (scale * scale)))
    s = (f8(q) @ f8(k).T).astype(np.float32)
    m_run = np.full((n, 1), -np.inf, dtype=np.float32)
    l_run = np.zeros((n, 1), dtype=np.float32)
    o = np.zeros((n, d), dtype=np.float32)
    with np.errstate(invalid="ignore", under="ignore"):
        for c in range(0, n, chunk):
            sl = slice(c, min(c + chunk, n))
            m_new = np.maximum(m_run, s[:, sl].max(axis=1, keepdims=True) * sc)
            alpha = np.exp2(m_run - m_new).astype(np.float32)
            p = np.exp2((f8(s[:, sl]) * f8(sc) - f8(m_new)).astype(np.float32)).astype(np.float32)
            l_run = l_run * alpha + p.sum(axis=1, keepdims=True, dtype=np.float32)
            o = o * alpha + (f8(p.astype(np.float16)) @ f8(v[sl])).astype(np.float32)
            m_run = m_new
    return (o * (np.float32(1) / l_run)).astype(np.float16)


def gelu_tanh_f32(x):
    """gemm.hip gelu_tanh in float32: x / (1 + exp2(t)), t = x fma(x x, c2, c1); exp2 and the reciprocal correctly rounded where the
    device is within one ulp"""
    x = np.asarray(x, dtype=np.float32)
    c1 = np.float32(-2.0) * np.float32(0.79788456080286535588) * np.float32(1.44269504088896340736)
    c2 = c1 * np.float32(0.044715)
    with np.errstate(over="ignore"):
        t = x * (f8(x * x) * f8(c2) + f8(c1)).astype(np.float32)
        return x * (1.0 / f8(np.float32(1) + np.exp2(f8(t)).astype(np.float32))).astype(np.float32)


def generic_gemm(A, W, bias, resid, epilogue, k_terms=None):
    """gemm_naive_kernel: one ascending f32 chain over k of exact products, + bias, the epilogue in f32, one rounding to f16.
    k_terms: how many of the K terms enter the sum (None: all; K - 1: a loop that ends one short)"""
    a, w = f8(np.asarray(A).astype(np.float16)), f8(np.asarray(W).astype(np.float16))
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for kk in range(a.shape[1] if k_terms is None else k_terms):
        acc = (f8(acc) + a[:, kk, None] * w[None, :, kk]).astype(np.float32)
    acc = acc + np.asarray(bias, dtype=np.float32)[None, :]
    if epilogue == 1:
        acc = gelu_tanh_f32(acc)
    if epilogue == 2:
        acc = acc + np.asarray(resid).astype(np.float16).astype(np.float32)
    return acc.astype(np.float16)


def generic_attention(q, k, v, lanes=64):
    """attention_naive_kernel for one head in float32: ascending chains for the scores, the product with 1 / sqrtf(d), the true
    maximum, exp2 of the rounded product with log2(e) (__expf), lane j % 64 sums its keys in ascending order and the lanes' sums
    meet in the wave's xor tree, an ascending chain of rounded products v_j p_j, the product with 1 / L, one rounding to f16.
    lanes: how many of the 64 lanes' sums enter L (64: the kernel)"""
    q, k, v = (np.asarray(a).astype(np.float16) for a in (q, k, v))
    n, d = q.shape
    s = np.zeros((n, n), np.float32)
    for e in range(d):
        s = (f8(s) + f8(q[:, e, None]) * f8(k[None, :, e])).astype(np.float32)
    s = s * (np.float32(1) / np.sqrt(np.float32(d)))
    x = s - s.max(axis=1, keepdims=True)
    with np.errstate(under="ignore"):
        p = np.exp2(f8(x * np.float32(1.44269504088896340736))).astype(np.float32)
    p[p < np.float32(2.0 ** -126)] = 0
    part = np.zeros((n, 64), np.float32)
    for j in range(n):
        part[:, j % 64] += p[:, j]
    part[:, lanes:] = 0
    o = 32
    while o:
        part = part + part[:, np.arange(64) ^ o]
        o >>= 1
    inv = np.float32(1) / part[:, :1]
    acc = np.zeros((n, d), np.float32)
    for j in range(n):
        acc = acc + v[j].astype(np.float32)[None, :] * p[:, j, None]
    return (acc * inv).astype(np.float16)


# ------------------------------------------------------------------------------------------------
# the inputs of the value-range tests (the GPU file runs the kernels on them, the host file the emulations)
# ------------------------------------------------------------------------------------------------
def gelu_sweep():
    """f16 pre-activations: steps of 1 / 64 on [-16, 16], EVERY f16 value on [-6, -2] (where 2^t grows from 2^6 to infinity), the
    two zeros, the largest subnormal and the smallest normal value, and magnitudes up to the largest finite one"""
    grid = np.arange(-1024, 1025) / 64.0
    dense = np.arange(0xC000, 0xC600 + 1, dtype=np.uint16).view(np.float16)          # -2.0 .. -6.0
    edge = [0.0, -0.0, 6.0e-8, -6.0e-8, 6.0976e-5, -6.0976e-5, 6.104e-5, -6.104e-5]
    far = [s * m for m in (32, 200, 1000, 30000, 65504) for s in (1, -1)]
    return np.concatenate([grid, f8(dense), edge, far]).astype(np.float16)


def gelu_biases(N):
    """bias 0 (the pre-activation is the f16 value itself), and f32 values in (-0.5, 0.5) that are no f16 numbers"""
    b = np.random.default_rng(N).uniform(-0.5, 0.5, N).astype(np.float32)
    b[b.astype(np.float16).astype(np.float32) == b] += np.float32(2.0 ** -20)
    return {"zero": np.zeros(N, dtype=np.float32), "f32": b}


LN_CLASSES = ["ratio0", "ratio1", "ratio4", "ratio16", "outlier", "near-constant"]


def layernorm_rows(M, H, seed, carried=4.0):
    """M rows of H values for a LayerNorm, cycling through LN_CLASSES: mean / std 0, 1, 4, 16; one feature 40 std away from the
    rest; std = 2^-6 of the mean (mean / std 64).  Every row is `carried` (what a bias adds in f32) + the f16 part returned (what an
    f16 activation holds): returns (part f16 [M][H], rows float64 [M][H] = carried + part, the class of every row)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 1, (M, H))
    cls = [LN_CLASSES[m % len(LN_CLASSES)] for m in range(M)]
    part = np.empty((M, H))
    for m, c in enumerate(cls):
        if c == "ratio0":
            part[m] = z[m] - carried
        elif c == "outlier":
            part[m] = z[m]
            part[m, (7 * m + 3) % H] += 40.0
        else:
            part[m] = z[m] * {"ratio1": carried, "ratio4": carried / 4, "ratio16": carried / 16, "near-constant": carried / 64}[c]
    part = part.astype(np.float16)
    return part, carried + f8(part), cls


SOFTMAX_LENS = [1, 16, 17, 127, 128, 129, 257, 512]
SOFTMAX_CASES = ["identical", "ahead-first", "ahead-last", "ahead-128", "ahead-per-query", "rising", "falling", "wide", "big-v", "subnormal-v"]


def softmax_case(case, n, d, seed=0):
    """q, k, v [n][d] f16 of one head (the kernels scale the scores by 1 / sqrt(d)):
    identical         all keys equal: the output is the mean of V
    ahead-*           one key at least 40 (natural-log units) ahead of every other: the first, the last, key 128 (the first of the
                      second 128-key chunk; the last key of a shorter sentence), a different one for every query
    rising / falling  the maximum grows (falls) by 180 natural-log units, more than 2^8 in exp2's, with every 128-key chunk
    wide              scaled scores spread over [-300, 300], the query's sign alternating
    big-v             |V| = 2^10 .. 2^14 with the sign alternating from key to key, under a spread-out softmax
    subnormal-v       V in the f16 subnormals"""
    rng = np.random.default_rng(1000 * n + d + seed)
    scale = 1 / np.sqrt(d)
    q = rng.normal(0, 1, (n, d))
    k = rng.normal(0, 1, (n, d))
    v = rng.normal(0, 1, (n, d))
    if case == "identical":
        k[:] = k[0]
    elif case.startswith("ahead"):
        # random sign vectors: s_i . s_j = d for i = j, a few sqrt(d) otherwise
        s = rng.choice([-1.0, 1.0], size=(n, d))
        target = {"ahead-first": np.zeros(n, dtype=int), "ahead-last": np.full(n, n - 1), "ahead-128": np.full(n, min(128, n - 1)),
                  "ahead-per-query": (7 * np.arange(n) + 3) % n}[case]
        amp = 8.0 if d == 32 else 5.0
        q = amp * s[target] + q / 8
        k = amp * s + k / 8
    elif case in ("rising", "falling"):
        chunk = np.arange(n) // 128
        level = (chunk - chunk.max() / 2) * 180.0 * (1 if case == "rising" else -1)
        q[:, 0] = 16
        k[:, 0] = level / (16 * scale)
    elif case == "wide":
        q[:, 0] = 16 * np.where(np.arange(n) % 2, -1, 1)
        k[:, 0] = rng.uniform(-300, 300, n) / (16 * scale)
    elif case == "big-v":
        q *= 1.7
        v = np.where(np.arange(n) % 2, -1.0, 1.0)[:, None] * 2.0 ** (10 + (np.arange(n)[:, None] + np.arange(d)[None, :]) % 5)
    elif case == "subnormal-v":
        q *= 1.7
        v *= 2.0 ** -17
    return q.astype(np.float16), k.astype(np.float16), v.astype(np.float16)


def generic_gemm_inputs(M, N, K, seed=0):
    """A [M][K] f16, W [N][K] f32 (to be stored in a file type), bias [N] f32, resid [M][N] f16: normal draws, the columns of W
    growing with k by a factor 2 over the row (a kernel that swaps, repeats or drops a k cannot pass), sums of size 1"""
    rng = np.random.default_rng(1000003 * M + 1009 * N + K + seed)
    A = rng.normal(0, 1, (M, K)).astype(np.float16)
    W = (rng.normal(0, 1, (N, K)) / np.sqrt(K) * (1 + np.arange(K) / K)).astype(np.float32)
    return A, W, rng.normal(0, 0.5, N).astype(np.float32), rng.normal(0, 1, (M, N)).astype(np.float16)


def generic_attention_inputs(lens, n_head, d_head):
    """qkv [T][3H] f16 for sentences of `lens`: Q a little wide, so that the softmax is neither flat nor one-hot"""
    rng = np.random.default_rng(sum(lens) * 131 + n_head * 17 + d_head)
    H = n_head * d_head
    qkv = rng.normal(0, 1, (sum(lens), 3 * H))
    qkv[:, :H] *= 1.7
    return qkv.astype(np.float16)
