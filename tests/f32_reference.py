"""Float64 restatements of the five operations of the f32 route (f32_route.hip), per-element error bounds derived from the roundings
the kernels perform (unit roundoff u = 2^-24: |fl(a) - a| <= u |a|, every f32 operation of the device rounds to nearest), NumPy float32
emulations of that arithmetic, and the inputs -- shared by test_gpu_f32_route.py (the kernels, on the GPU) and test_f32_bounds_host.py
(the emulations and deliberately wrong ones, without a GPU).  Inputs are kept NORMAL f32 numbers of ordinary size, so that whether the
device flushes subnormal operands or results is not part of the question; no bound below has a term for it."""
import functools

import numpy as np

import layer_reference as ref
from layer_reference import U32 as U, f8

# Device tanhf, in ulp of its f32 result.  The toolchain ships no figure for it, so it was measured on an MI355X against float64
# tanh over f32_gelu's arguments for gelu_sweep()'s pre-activations (the f16 sweep plus both bias vectors of gelu_biases(64), 461 312
# arguments): worst TANHF_ULP_MEASURED.  A sweep samples the function and does not prove it: the bound takes twice that.
TANHF_ULP_MEASURED = 1.244          # (at arg = -0.6614: -0.5793053 for -0.57930522; median 0.06, 99.9 % below 0.73)
TANHF_ULP = 2 * TANHF_ULP_MEASURED
# expf: not measured; the device library is built to OpenCL's full-profile requirement for exp, 3 ulp
EXPF_ULP = 3.0


def spacing32(a):
    """the distance between neighbouring f32 numbers at |a| (one ulp)"""
    return f8(np.spacing(np.abs(f8(a)).astype(np.float32)))


def f4(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------
# mat-mul
# ------------------------------------------------------------------------------------------------
EPI_BIAS, EPI_GELU, EPI_RESID = 0, 1, 2


def matmul(A, W, bias, resid=None):
    """A W^T + bias (+ resid) in float64"""
    return f8(A) @ f8(W).T + f8(bias) + (0 if resid is None else f8(resid))


def matmul_bound(A, W, bias, resid=None):
    """|device - (A W^T + bias (+ resid))| <= (K + c) u S + u |A W^T + bias| (+ u |want|), S = sum_k |a_k w_k| per element:
      - the accumulator is a chain of K fused multiply-adds in f32 (v_mfma_f32_32x32x2_f32; the lanes of a partial reduction tile add
        exact zeros): K roundings, and whatever the order the error of the sum is at most g_K S with g_K = K u / (1 - K u);
      - the epilogue adds the bias in f32: one rounding of acc + bias, at most u (|A W^T + bias| + g_K S).  Without a residual that
        sum is the result, u |want|;
      - with a residual one more addition and rounding, u |want| -- and the bias term stays a fraction of the sum it rounded, which a
        residual that cancels it does not scale down.
    g_K (1 + 2 u) <= (K + 1) u as long as K^2 u <= 1 (K <= 4096); c = 2 leaves that room twice.  No factor for the matrix cores: the
    f32 form multiplies and adds f32 numbers, there is nothing narrower inside it to round to.
    Returns (bound, want, S)."""
    K = np.shape(A)[1]
    S = np.abs(f8(A)) @ np.abs(f8(W)).T
    pre = matmul(A, W, bias)
    want = pre if resid is None else pre + f8(resid)
    return (K + 2) * U * S + U * np.abs(pre) + (0 if resid is None else U * np.abs(want)), want, S


def gelu_bound(pre, dpre):
    """|device - gelu(pre)| for f32_gelu, `pre` the float64 pre-activation and dpre the most the device's f32 one differs from it (to
    first order it does not matter at which of the two the terms below are taken):
      - |gelu'| <= 1.13 everywhere: 1.13 dpre;
      - arg = c x (1 + 0.044715 x^2): the two constants round to f32 (u each) and, unfused, c x, 0.044715 x, its product with x, the
        sum with 1 (every error of the second factor is a smaller fraction of the sum than of x^2) and the last product round once
        each: |d arg| <= 7 u |arg|, which tanh turns into (1 - tanh^2) 7 u |arg|;
      - tanhf: TANHF_ULP ulp of its result;
      - s = 1 + tanh rounds once: u |s|.  The ERROR OF s is the sum of the three, an absolute quantity: where x is negative and tanh
        near -1 the ulp of tanh stays 2^-24 while s itself goes to 0, and the bound keeps that cancellation inside it;
      - 0.5 x is exact, its product with s rounds once: 0.5 |x| ds + u |gelu|."""
    x = f8(pre)
    arg = 0.7978845608028654 * x * (1 + 0.044715 * x * x)
    th = np.tanh(arg)
    ds = (1 - th * th) * 7 * U * np.abs(arg) + TANHF_ULP * spacing32(th) + U * np.abs(1 + th)
    return 1.13 * f8(dpre) + 0.5 * np.abs(x) * ds + U * np.abs(ref.gelu(x))


def gemm_bound(A, W, bias, resid, epilogue):
    """(bound, want) of one call of the kernel under `epilogue`; GELU: the bound is about the float64 pre-activation, which is what
    the device's own differs from by at most matmul_bound"""
    bound, want, _ = matmul_bound(A, W, bias, resid if epilogue == EPI_RESID else None)
    if epilogue == EPI_GELU:
        return gelu_bound(want, bound), ref.gelu(want)
    return bound, want


def fma_chain(A, W, bias, resid=None):
    """The mat-mul as ONE correctly rounded f32 fma chain per element in ascending k (the product of two f32 is exact in float64 and
    the sum rounds once to f32, up to a double rounding of 2^-29 ulp; index_reference.f32_chain_scores is the model), then the f32
    additions of the epilogue.  If the device's bits equal this, the order inside the matrix cores is known."""
    a, w = f8(f4(A)), f8(f4(W))
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc = (f8(acc) + a[:, k, None] * w[None, :, k]).astype(np.float32)
    acc = acc + f4(bias)[None, :]
    return acc if resid is None else acc + f4(resid)


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K):
    """A [M][K], W [N][K], bias [N], resid [M][N] as f32: normal draws, the columns of W growing with k by a factor 2 over the row (a
    kernel that swaps, repeats or drops a k cannot pass), sums of size 1.  Read-only."""
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    A = f4(rng.normal(0, 1, (M, K)))
    W = f4(rng.normal(0, 1, (N, K)) / np.sqrt(K) * (1 + np.arange(K) / K))
    bias = f4(rng.normal(0, 0.5, N))
    resid = f4(rng.normal(0, 1, (M, N)))
    for a in (A, W, bias, resid):
        assert (np.abs(a) >= 2.0 ** -100).all()
        a.setflags(write=False)
    return A, W, bias, resid


# every M of {1, 31, 32, 33, 63, 64, 65, 129}, N of {1, 3, 4, 5, 31, 33, 63, 64, 65, 100, 130} and K of {1, 2, 3, 4, 5, 15, 16, 17, 18, 31,
# 33, 100, 384} appears; the corners and one model shape first
GEMM_SHAPES = [(1, 1, 1), (65, 65, 17), (33, 130, 100), (129, 100, 33), (130, 1536, 384),
               (1, 3, 2), (1, 4, 3), (1, 5, 4), (1, 64, 16), (1, 130, 5), (31, 1, 15), (31, 31, 31), (31, 33, 18), (32, 4, 4), (32, 63, 15),
               (32, 64, 16), (33, 3, 1), (33, 5, 17), (33, 65, 33), (63, 31, 2), (63, 63, 100), (63, 100, 3), (64, 1, 384), (64, 64, 16),
               (64, 65, 5), (64, 130, 18), (65, 3, 31), (65, 4, 100), (65, 33, 384), (65, 64, 1), (129, 5, 16), (129, 31, 4), (129, 63, 17),
               (129, 130, 15), (129, 65, 384), (31, 100, 384), (32, 33, 3), (63, 4, 18), (1, 1, 384), (129, 1, 1)]


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def attention(q, k, v):
    """softmax(q k^T / sqrt(d)) v for one head in float64"""
    q, k, v = f8(q), f8(k), f8(v)
    sc = q @ k.T / np.sqrt(q.shape[1])
    p = np.exp(sc - sc.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True) @ v


def softmax_bound(q, k, v, u=U, exp_ulp=EXPF_ULP):
    """layer_reference.softmax_bound with the unit roundoff as a parameter, for a kernel that keeps every number in one format of unit
    roundoff u, subtracts the TRUE maximum and divides once at the end (f32_attention_kernel): no rescalings, no narrower P.  One head,
    q, k, v [n][d]; to first order, with p_j = exp(s_j - max), L = sum p, w = p / L:
      - s_j = (sum_e k_e q_e) * scale: a chain of d fused multiply-adds, d u sum |k q|; scale = 1 / sqrtf(d), two roundings, and the
        product a third: (d + 3) u (|q| . |k_j|) scale in all;
      - s_j - max rounds once, u |s_j - max|; the maximum's own error multiplies every p by the same factor and cancels in p / L;
        expf: exp_ulp ulp, 2 exp_ulp u of p_j.  Relative to p_j: eps_j;
      - L is a sum of the n numbers p_j in some order, n u; 1 / L rounds once; the output is a chain of n fused multiply-adds,
        n u sum p |v|, and its product with 1 / L rounds once: (2 n + 2) u sum w |v|.
    |dw_j| <= w_j eps_j + w_j sum_k w_k eps_k.  Returns (bound, want)."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    scale = 1 / np.sqrt(d)
    sc = q @ k.T * scale
    mx = sc.max(axis=1, keepdims=True)
    eps = (d + 3) * u * (np.abs(q) @ np.abs(k).T) * scale + u * (mx - sc) + 2 * exp_ulp * u
    p = np.exp(sc - mx)
    w = p / p.sum(axis=1, keepdims=True)
    dw = w * eps + w * (w * eps).sum(axis=1, keepdims=True)
    return dw @ np.abs(v) + (2 * n + 2) * u * (w @ np.abs(v)), w @ v


def attention_packed(qkv, lens, n_head, d_head, bound=False):
    """qkv [T][3H] of packed sentences -> the float64 context rows [T][H] (and their bounds)"""
    H = n_head * d_head
    want, bnd = np.zeros((len(qkv), H)), np.zeros((len(qkv), H))
    t0 = 0
    for n in lens:
        for h in range(n_head):
            sl = slice(h * d_head, (h + 1) * d_head)
            q, k, v = (qkv[t0:t0 + n, i * H:(i + 1) * H][:, sl] for i in range(3))
            if bound:
                bnd[t0:t0 + n, sl], want[t0:t0 + n, sl] = softmax_bound(q, k, v)
            else:
                want[t0:t0 + n, sl] = attention(q, k, v)
        t0 += n
    return (want, bnd) if bound else want


@functools.lru_cache(maxsize=None)
def attention_inputs(lens, n_head, d_head):
    """qkv [T][3H] f32 for sentences of `lens` (a tuple): Q a little wide, so that the softmax is neither flat nor one-hot.  Read-only."""
    rng = np.random.default_rng(sum(lens) * 131 + n_head * 17 + d_head)
    H = n_head * d_head
    qkv = rng.normal(0, 1, (sum(lens), 3 * H))
    qkv[:, :H] *= 1.7
    qkv = f4(qkv)
    qkv.setflags(write=False)
    return qkv


# ------------------------------------------------------------------------------------------------
# LayerNorm, embedding
# ------------------------------------------------------------------------------------------------
def layernorm_bound(v, g, want):
    """layer_reference.layernorm_bound for two-pass statistics with every rounding of the output in f32: v - mean, its product with
    1 / std and the one with gamma round once each (3 u of gamma (v - mean) / std), the sum with beta once (u |want|); sqrtf and the
    division behind 1 / std are two roundings more of every normalised value."""
    v, g = f8(v), f8(g)
    mu = v.mean(axis=1, keepdims=True)
    sd = np.sqrt(((v - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5)
    rounding = 5 * U * np.abs((v - mu) / sd * g) + U * np.abs(want)
    return ref.layernorm_bound(v, g, want, one_pass=False, rounding=rounding)


def embed_rows(word, type_, pos, tokens, lens):
    """pos[p] + (type[0] + word[id]) in float64, and the most the two f32 additions can be off"""
    p = np.concatenate([np.arange(n) for n in lens])
    inner = f8(type_)[0][None, :] + f8(word)[tokens]
    rows = f8(pos)[p] + inner
    return rows, U * (np.abs(inner) + np.abs(rows))


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
def pool(rows, pooling, normalize):
    """rows [n][H] float64 -> the sentence's embedding as bert_hip.h defines it"""
    y = rows[0] if pooling == "cls" else rows.mean(axis=0)
    return y / np.sqrt((y * y).sum()) if normalize else y


def pool_bound(rows, pooling, normalize):
    """f32_pool_normalize_kernel on the f32 rows [n][H] of one sentence:
      - mean: every term is x_t * (1 / n) -- 1 / n rounds once, the product once -- and the n terms are added one after the other:
        dy <= (n + 2) u mean_t |x_t|; CLS: the stored row, dy = 0;
      - raw: that is all.  Normalised: y / ||y|| moves by dy / ||y|| and, through the norm, by |want| ||dy|| / ||y||; the sum of the H
        squares (each rounds once, the sum in some order) is off by (H + 1) u of itself, half that in the norm; sqrtf, the division
        and the product with y round once each: ((H + 1) / 2 + 3) u |want|.  No epsilon under the root.
    Returns (bound, want)."""
    rows = f8(rows)
    n, H = rows.shape
    want = pool(rows, pooling, normalize)
    dy = np.zeros(H) if pooling == "cls" else (n + 2) * U * np.abs(rows).mean(axis=0)
    if not normalize:
        return dy, want
    y = rows[0] if pooling == "cls" else rows.mean(axis=0)
    norm = np.sqrt((y * y).sum())
    return dy / norm + np.abs(want) * (np.sqrt((dy * dy).sum()) / norm + ((H + 1) / 2 + 3) * U), want


# ------------------------------------------------------------------------------------------------
# NumPy float32 emulations of the device arithmetic the bounds are about
# ------------------------------------------------------------------------------------------------
def gelu_f32(x):
    """f32_gelu, every operation rounded to f32 where the unfused device code rounds, tanh correctly rounded"""
    x = f4(x)
    c, a = np.float32(0.79788456080286535588), np.float32(0.044715)
    with np.errstate(over="ignore"):
        arg = (c * x) * (np.float32(1) + (a * x) * x)
    return np.float32(0.5) * x * (np.float32(1) + np.tanh(f8(arg)).astype(np.float32))


def matmul_pairwise_f32(A, W, bias, resid=None):
    """f32 products (rounded), NumPy's pairwise f32 sum over k, the epilogue's f32 additions"""
    acc = (f4(A)[:, None, :] * f4(W)[None, :, :]).sum(axis=2, dtype=np.float32) + f4(bias)[None, :]
    return acc if resid is None else acc + f4(resid)


def attention_f32(q, k, v, scale=None):
    """f32_attention_kernel for one head: f32 scores (BLAS order), true maximum, f32 exponentials, sum, reciprocal, f32 output sums"""
    q, k, v = f4(q), f4(k), f4(v)
    scale = np.float32(1) / np.sqrt(np.float32(q.shape[1])) if scale is None else np.float32(scale)
    s = (q @ k.T) * scale
    p = np.exp(s - s.max(axis=1, keepdims=True))
    inv = np.float32(1) / p.sum(axis=1, keepdims=True, dtype=np.float32)
    return (p @ v) * inv


def layernorm_two_pass_f32(v, g, b):
    """f32_layernorm_row: f32 mean, f32 sum of the centred squares, 1 / sqrtf, gamma * ((v - mean) * rstd) + beta"""
    v, g, b = f4(v), f4(g), f4(b)
    H = np.float32(v.shape[1])
    mean = v.sum(axis=1, keepdims=True, dtype=np.float32) / H
    d = v - mean
    rstd = np.float32(1) / np.sqrt((d * d).sum(axis=1, keepdims=True, dtype=np.float32) / H + np.float32(1e-5))
    return g * (d * rstd) + b


def pool_f32(rows, pooling, normalize, waves=4):
    """f32_pool_normalize_kernel on one sentence; waves: how many of the four wave sums enter the norm (4: the kernel)"""
    rows = f4(rows)
    n, H = rows.shape
    if pooling == "cls":
        y = rows[0].copy()
    else:
        invn = np.float32(1) / np.float32(n)
        y = np.zeros(H, np.float32)
        for t in range(n):
            y = y + rows[t] * invn
    if not normalize:
        return y
    sq = y * y
    # thread tid sums the features tid, tid + 256, ...; wave w is threads 64 w .. 64 w + 63
    red = [sum((sq[tid::256].sum(dtype=np.float32) for tid in range(64 * w, 64 * w + 64) if tid < H), np.float32(0)) for w in range(4)]
    total = (red[0] + red[1]) + (red[2] + red[3]) if waves == 4 else sum(red[:waves], np.float32(0))
    return y * (np.float32(1) / np.sqrt(total))


@functools.lru_cache(maxsize=None)
def layernorm_inputs(H, M=24):
    """layer_reference.layernorm_rows as f32 rows (4.0 + the f16 part: exact in f32), gamma, beta; every class is in the domain of
    two-pass statistics.  Returns (rows f32 [M][H], gamma, beta, classes)."""
    part, _, cls = ref.layernorm_rows(M, H, 7000 + H)
    rng = np.random.default_rng(H)
    v = np.float32(4.0) + part.astype(np.float32)
    g, b = f4(1 + rng.normal(0, 0.1, H)), f4(rng.normal(0, 0.1, H))
    for a in (v, g, b):
        a.setflags(write=False)
    return v, g, b, cls
