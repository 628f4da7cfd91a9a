"""The batch route's GELU, softmax and LayerNorm outside the comfortable corner of N(0, 1) activations, each against float64 and a
per-element bound DERIVED from the roundings the kernel performs (layer_reference.py: gelu_bound, softmax_bound, layernorm_bound; no
bound comes from a measurement).  test_value_bounds_host.py holds NumPy emulations of the device arithmetic to the same bounds on the
same inputs, without a GPU.  Every test prints the worst fraction of its bound; the docstrings record them."""
import functools

import numpy as np
import pytest

from bert_cpp_amd import pybert

import layer_reference as ref
from test_gpu_latency_kernels import _natural_order, _qkv_weights, _same_bits

pytestmark = pytest.mark.gpu


def _inside(got, want, bound, what):
    err = np.abs(ref.f8(got) - want)
    frac = float((err / bound).max())
    print(f"{what}: worst err / bound {frac:.3f} (err {err.max():.3e})")
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, (what, frac, len(bad), bad[:5].tolist(), [float(want[tuple(i)]) for i in bad[:5]], [float(ref.f8(got)[tuple(i)]) for i in bad[:5]])
    return frac


# ------------------------------------------------------------------------------------------------
# B1: the GELU epilogue
# ------------------------------------------------------------------------------------------------
def _check_gelu(got, pre, what, starts_from_f16=True):
    """got f16 against float64 tanh-GELU of the f32 pre-activations: the derived bound, and the three properties without one.
    starts_from_f16: the kernel rounds the pre-activation to f16 and evaluates the GELU on that (gelu_pk16h), or the pre-activation
    is an f16 number anyway; a kernel that evaluates in f32 on a pre-activation between two f16 numbers owes x only through the bound"""
    pre = np.asarray(pre, dtype=np.float32)
    assert np.isfinite(got).all(), (what, "NaN or Inf at", pre[~np.isfinite(got)][:5].tolist())
    _inside(got, ref.gelu(ref.f8(pre)), ref.gelu_bound(pre), what)
    assert (ref.f8(got)[pre < 0] <= 0).all(), (what, "positive for", pre[(pre < 0) & (ref.f8(got) > 0)][:5].tolist())
    same = ref.gelu_rounds_to_x(pre) & starts_from_f16
    x = pre.astype(np.float16)
    neq = same & (got.view(np.uint16) != x.view(np.uint16))
    assert not neq.any(), (what, "not x itself at", pre[neq][:5].tolist(), got[neq][:5].tolist())


@pytest.mark.parametrize("bias", ["zero", "f32"])
@pytest.mark.parametrize("impl", [0, 1, 3], ids=["mfma", "naive", "tile256"])
def test_gelu_epilogue_of_the_gemms(impl, bias):
    """W is zero but for W[n][0] = 1, so the pre-activation is A[m][0] + bias[n] exactly (one f32 addition); the other columns of A
    are random and meet zeros.  A[m][0] sweeps layer_reference.gelu_sweep() in calls of 512 rows.  gemm.hip and the generic kernel
    evaluate the GELU in f32, gemm256.hip in packed f16 (gelu_pk16h).  Worst measured fraction of the bound on the MI355X: f32 forms
    0.18, and 0.50 on the smallest subnormal (the rounding of the result); gemm256 0.977, at -4.027 where t rounds up to 16 and the
    result is flushed (6.16e-5 of the 6.31e-5 allowed there; 0.96 at -4.031, the next value down), 0.39 above the flush.  The
    emulation in test_value_bounds_host.py gives the same 0.977."""
    N, K = (256, 128) if impl == 3 else (64, 64)
    W = np.zeros((N, K), dtype=np.float16)
    W[:, 0] = 1
    b = ref.gelu_biases(N)[bias]
    sweep = ref.gelu_sweep()
    rng = np.random.default_rng(impl)
    for m0 in range(0, len(sweep), 512):
        A = rng.normal(0, 1, (len(sweep[m0:m0 + 512]), K)).astype(np.float16)
        A[:, 0] = sweep[m0:m0 + 512]
        got = pybert.test_gemm(A, W.view(np.uint8), 1, N, b, None, 1, impl)
        pre = A[:, :1].astype(np.float32) + b[None, :]
        plain = pybert.test_gemm(A, W.view(np.uint8), 1, N, b, None, 0, impl)
        _same_bits(plain, pre.astype(np.float16), "the pre-activation is exact")
        _check_gelu(got, pre, f"impl {impl} bias {bias} rows {m0}", starts_from_f16=impl == 3 or bias == "zero")


@pytest.mark.parametrize("rebuild", [False, True], ids=["plain-residual", "rebuilt-residual"])
def test_gelu_epilogue_of_the_layernorm_fold(rebuild, M=33, K1=128, H=256, N2=2048):
    """The consuming mat-mul of the fold (row scale, then gelu_pk16h): its pre-activation is not exact, but the same pair with the
    bias epilogue returns it as the f16 value the GELU starts from.  b2 carries the sweep, LayerNorm(u) W2^T spreads the rows around it.
    Worst measured fraction of the bound: 0.977 (the flush at -4.027), both residual forms."""
    rng = np.random.default_rng(N2 + rebuild)
    sweep = ref.gelu_sweep()
    sweep = sweep[np.abs(ref.f8(sweep)) < 40000]
    b2 = np.resize(np.concatenate([sweep[2049:], sweep[:2049:4]]), N2).astype(np.float32)       # every value of [-6, -2] first
    A1 = rng.normal(0, 1, (M, K1)).astype(np.float16)
    W1 = (rng.normal(0, 1, (H, K1)) / np.sqrt(K1)).astype(np.float16)
    b1 = rng.normal(0, 0.3, H).astype(np.float32)
    r = rng.normal(0, 1, (M, H)).astype(np.float16)
    rg, rb = ((1 + rng.normal(0, 0.2, H)).astype(np.float32), rng.normal(0, 0.2, H).astype(np.float32)) if rebuild else (None, None)
    W2 = (rng.normal(0, 1, (N2, H)) / np.sqrt(H) / 8).astype(np.float16)
    g, be = (1 + rng.normal(0, 0.2, H)).astype(np.float32), rng.normal(0, 0.3, H).astype(np.float32)
    _, pre, _ = pybert.test_gemm_lnfold(A1, W1, b1, r, rg, rb, W2, b2, g, be, 0)
    _, got, _ = pybert.test_gemm_lnfold(A1, W1, b1, r, rg, rb, W2, b2, g, be, 1)
    assert np.isfinite(pre).all() and len(np.unique(pre)) > 5000
    _check_gelu(got, pre.astype(np.float32), f"fold rebuild {rebuild}")


@pytest.mark.parametrize("bias", ["f16", "f32"])
def test_gelu_of_the_latency_route_s_up_projection(bias, M=33, H=256, I=2560):
    """skinny.hip SK_UP: LayerNorm 1 with gamma = 0 leaves y = beta for every token, W1[n][0] = 1 picks y[0] = 0, and b1 carries the
    sweep: as f16 values, and moved off them by f32 amounts.  Worst measured fraction of the bound: 0.977 (the flush at -4.027), both."""
    rng = np.random.default_rng(I)
    sweep = ref.gelu_sweep()
    b1 = np.resize(np.concatenate([sweep[2049:], sweep[:2049:2]]), I).astype(np.float32)
    if bias == "f32":
        b1 = (b1 + rng.uniform(-0.01, 0.01, I).astype(np.float32) * np.maximum(np.abs(b1), 1)).astype(np.float32)
        b1 = np.clip(b1, -65504, 65504)
    ctx, x = rng.normal(0, 1, (M, H)).astype(np.float16), rng.normal(0, 1, (M, H)).astype(np.float16)
    Wo = (rng.normal(0, 1, (H, H)) / np.sqrt(H)).astype(np.float16)
    W1 = np.zeros((I, H), dtype=np.float16)
    W1[:, 0] = 1
    W2 = (rng.normal(0, 1, (H, I)) / np.sqrt(I) / 256).astype(np.float16)
    zeros, be1 = np.zeros(H, dtype=np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    be1[0] = 0
    _, p = pybert.test_skinny_tail(ctx, x, Wo.view(np.uint8), W1.view(np.uint8), W2.view(np.uint8), 1, I, zeros, zeros, be1, b1, zeros,
                                   np.ones(H, dtype=np.float32), zeros, parts=True)
    _same_bits(p["y"], np.broadcast_to(be1.astype(np.float16), (M, H)).copy(), "y is beta")
    # (the accumulator holds y W1^T = +0 when the bias joins it: a bias of -0 gives +0)
    _check_gelu(_natural_order(p["ff"]), np.broadcast_to(np.float32(0) + b1, (M, I)), f"skinny up-projection bias {bias}")


# ------------------------------------------------------------------------------------------------
# B2: softmax
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _softmax_heads(n, d):
    """every case of layer_reference.SOFTMAX_CASES as one head of a sentence of n tokens: qkv [n][3 H], want and bound [n][H]"""
    cases = [ref.softmax_case(c, n, d) for c in ref.SOFTMAX_CASES]
    qkv = np.concatenate([np.concatenate([c[i] for c in cases], axis=1) for i in range(3)], axis=1)
    both = [ref.softmax_bound(q, k, v, 1 / np.sqrt(d)) for q, k, v in cases]
    return qkv, np.concatenate([w for _, w in both], axis=1), np.concatenate([b for b, _ in both], axis=1)


@pytest.mark.parametrize("impl", [0, 1], ids=["mfma", "naive"])
@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("n", ref.SOFTMAX_LENS)
def test_softmax_of_the_attention_kernel(impl, d_head, n):
    """attention.hip (one 128-key chunk up to 128 tokens, the online form with the running maximum beyond) and the generic kernel:
    identical keys, one key far ahead (first, last, first of the second chunk, another per query), maxima that rise or fall by
    more than 2^8 from chunk to chunk, scores of +-300, |V| up to 2^14 with alternating signs, subnormal V -- ten heads of one
    sentence.  The bound weighs every key's error by |V| (3.8 is inside it on the big-v head, 3e-8 is half of it on the subnormal one).
    Worst measured fractions of the bound on the MI355X, attention.hip / generic kernel: identical 0.21 / 0.21, rising and falling
    0.42 / 0.28, wide 0.10 / 0.08, big-v 0.34 / 0.24, subnormal-v 0.49 / 0.49 (the rounding of the result); the ahead-* heads are exact.
    attention.hip's figures are those of the float32 emulation in test_value_bounds_host.py."""
    qkv, want, bound = _softmax_heads(n, d_head)
    got = pybert.test_attention(qkv, np.array([0, n], dtype=np.int32), len(ref.SOFTMAX_CASES), d_head, impl)
    assert np.isfinite(got).all()
    for h, case in enumerate(ref.SOFTMAX_CASES):
        sl = slice(h * d_head, (h + 1) * d_head)
        _inside(got[:, sl], want[:, sl], bound[:, sl], f"impl {impl} d {d_head} n {n} {case}")


@pytest.mark.parametrize("n_head", [8, 12])
def test_softmax_of_projection_plus_attention(n_head, d=32):
    """bert_hip_test_qkv_attention in all its forms on Q, K, V that are features of x times powers of two (W: +-2^k on a permutation,
    bias 0: the projection is exact but for V's underflow, which the reference repeats): sentences of identical rows, of random sign
    vectors (every query's own key ahead by 40 and more once the head scales them up), of rows with alternating signs; heads that
    scale Q K^T by 1, 1 / 4, 64, 1 / 2 and V by 1, 2^12 (2^11 .. 2^13 under a spread-out softmax, the signs alternating in the sentences
    that alternate), 1, 2^-20 (subnormal).  The fused
    forms have the bits of the mat-mul + attention pair.  Worst measured fraction of the bound: 0.496 (the subnormal heads)."""
    H = n_head * d
    rng = np.random.default_rng(n_head)
    lens = [128, 17, 127, 16, 1, 64, 33]
    kinds = ["signs", "same", "alternating", "signs", "same", "alternating", "signs"]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = np.empty((int(cu[-1]), H))
    for b, kind in enumerate(kinds):
        n = lens[b]
        rows = rng.choice([-1.0, 1.0], size=(n, H)) + rng.integers(-2, 3, size=(n, H)) / 16.0
        if kind == "same":
            rows[:] = rows[0]
        elif kind == "alternating":
            rows = np.abs(rows) * np.where(np.arange(n) % 2, -1.0, 1.0)[:, None]
        x[cu[b]:cu[b + 1]] = rows
    x = x.astype(np.float16)
    W = np.zeros((3 * H, H))
    scales = [(1.0, 1.0, 1.0), (0.5, 0.5, 2.0 ** 12), (8.0, 8.0, 1.0), (1.0, 0.5, 2.0 ** -20)]
    for h in range(n_head):
        a, bb, c = scales[h % 4]
        for e in range(d):
            W[h * d + e, h * d + e] = a
            W[H + h * d + e, h * d + e] = bb
            W[2 * H + h * d + e, h * d + (e + 5) % d] = -c if e % 3 == 0 else c
    W = W.astype(np.float16)
    bias = np.zeros(3 * H, dtype=np.float32)
    qkv = (ref.f8(x) @ ref.f8(W).T).astype(np.float16)
    want, bound = np.empty((len(x), H)), np.empty((len(x), H))
    for b in range(len(lens)):
        for h in range(n_head):
            rows, sl = slice(cu[b], cu[b + 1]), slice(h * d, (h + 1) * d)
            bound[rows, sl], want[rows, sl] = ref.softmax_bound(qkv[rows, sl], qkv[rows, H + h * d:H + (h + 1) * d],
                                                                qkv[rows, 2 * H + h * d:2 * H + (h + 1) * d], 1 / np.sqrt(d))
    # the cases are there: a head with every query's own key 40 ahead, |V| of 2^11 and more, subnormal V
    sc = np.sort(ref.f8(qkv[:128, 2 * d:3 * d]) @ ref.f8(qkv[:128, H + 2 * d:H + 3 * d]).T / np.sqrt(d), axis=1)
    assert (sc[:, -1] - sc[:, -2]).min() >= 40 and 250 < sc.max() < 450, (float((sc[:, -1] - sc[:, -2]).min()), float(sc.max()))
    assert np.abs(ref.f8(qkv[:, 2 * H + d:2 * H + 2 * d])).min() >= 2.0 ** 11
    assert 0 < np.abs(ref.f8(qkv[:, 2 * H + 3 * d:2 * H + 4 * d])).max() < 6.1e-5
    split = pybert.test_qkv_attention(x, cu, n_head, d, W.view(np.uint8), 1, bias, 0)
    _inside(split, want, bound, f"n_head {n_head} mat-mul + attention")
    for mode in (2, 3, 4, 5):
        got = pybert.test_qkv_attention(x, cu, n_head, d, W.view(np.uint8), 1, bias, mode)
        _same_bits(got, split, f"mode {mode} against mat-mul + attention")


# ------------------------------------------------------------------------------------------------
# B3: LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln_params(rng, H):
    return (1 + rng.normal(0, 0.1, H)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)


def _by_class(got, want, bound, cls, what):
    err = np.abs(ref.f8(got) - want)
    for c in ref.LN_CLASSES:
        rows = [m for m, k in enumerate(cls) if k == c]
        if rows:
            print(f"  {what} {c}: worst err / bound {(err[rows] / bound[rows]).max():.3f} (err {err[rows].max():.2e}, bound {bound[rows].max():.2e})")
    _inside(got, want, bound, what)


@pytest.mark.parametrize("impl", [0, 1], ids=["five-kernels", "layer_tail"])
@pytest.mark.parametrize("H", [256, 384])
def test_layernorm_of_the_layer_tail(impl, H, M=33, I=256):
    """ctx = 0, bo = 4 and x carry rows of mean / std 0, 1, 4, 16, 64 (near-constant) and rows with one feature 40 std out into
    LayerNorm 1; W1 = W2 = 0 makes the feed-forward part vanish, so the output is LayerNorm 2 of y, a benign row, and
    LayerNorm 1's error passes through it to first order (layernorm_input_term).  layer_tail.hip forms the variance in one pass, the
    LayerNorm kernel of the five-kernel route in two: both are held to the one-pass bound.  Worst measured fractions of the bound,
    layer_tail.hip: 0.27 at mean / std 0, 0.25 at 1, 0.17 at 4, 0.03 at 16, 0.002 near-constant, 0.30 outlier; five kernels (the f16
    rounding of the sum in front of LayerNorm 1 is most of their bound): 0.22, 0.20, 0.22, 0.18, 0.11, 0.24."""
    part, rows, cls = ref.layernorm_rows(M, H, H + impl)
    rng = np.random.default_rng(H)
    (g1, be1), (g2, be2) = _ln_params(rng, H), _ln_params(rng, H)
    Wo = (rng.normal(0, 1, (H, H)) / np.sqrt(H)).astype(np.float16)
    zw1, zw2 = np.zeros((I, H), dtype=np.float16), np.zeros((H, I), dtype=np.float16)
    bo = np.full(H, 4.0, dtype=np.float32)
    got = pybert.test_layer_tail(np.zeros((M, H), dtype=np.float16), part, Wo.view(np.uint8), zw1.view(np.uint8), zw2.view(np.uint8), 1, I,
                                 bo, g1, be1, np.zeros(I, dtype=np.float32), np.zeros(H, dtype=np.float32), g2, be2, impl)
    y = ref.layernorm(rows, ref.f8(g1), ref.f8(be1))
    # (0 + bo + x in f32: two additions; the five-kernel route stores that sum as f16 for its LayerNorm kernel: half an f16 ulp more)
    dv = 2 * ref.U32 * np.abs(rows) + (0.5 * ref.ulp16(rows) if impl == 0 else 0.0)
    dy = ref.layernorm_bound(rows, g1, y, one_pass=True) + ref.layernorm_input_term(rows, g1, dv)
    want = ref.layernorm(y, ref.f8(g2), ref.f8(be2))
    bound = ref.layernorm_bound(y, g2, want, one_pass=True) + ref.layernorm_input_term(y, g2, dy)
    assert np.isfinite(got).all()
    _by_class(got, want, bound, cls, f"tail impl {impl} H {H}")


@pytest.mark.parametrize("rebuild", [False, True], ids=["plain-residual", "rebuilt-residual"])
@pytest.mark.parametrize("H", [256, 768])
def test_layernorm_folded_into_the_gemms_on_hard_rows(H, rebuild, M=33, K1=128):
    """The fold's statistics (partial sums in the producing mat-mul's epilogue, ln_rows_finalize: one pass) and the consuming mat-mul
    with W2 = identity, gamma a power of two per feature, beta = b2 = 0: out = (u - mean) gamma / std, LayerNorm(u) itself, against
    float64 on the u the pair returned.  Besides layernorm_bound: the extra k-step holds mean and std as hi / lo f16 pairs against
    hi / lo sums of the folded weights (2^-20 of |mean| gamma / std), and the f32 accumulation of the nine products that are not
    exactly zero.  plain residual: u = b1 + r, all classes of rows in one call; rebuilt residual: u = LayerNorm(r) rg + (rb + b1),
    one class per call.  Worst measured fractions of the bound (H = 256 / 768, plain residual): 0.47 / 0.42 at mean / std 0,
    0.43 / 0.36 at 1, 0.26 / 0.14 at 4, 0.04 / 0.01 at 16, 0.005 / 0.002 near-constant (mean / std 67 / 64), 0.39 / 0.22 outlier;
    rebuilt residual: 0.34 / 0.14, 0.44 / 0.37, 0.26 / 0.14, 0.04 / 0.01, 0.005 / 0.002, 0.24 / 0.13."""
    rng = np.random.default_rng(H + rebuild)
    A1 = np.zeros((M, K1), dtype=np.float16)
    W1 = (rng.normal(0, 1, (H, K1)) / np.sqrt(K1)).astype(np.float16)
    W2 = np.eye(H, dtype=np.float16)
    g = (2.0 ** rng.integers(-1, 2, H)).astype(np.float32)
    zeros = np.zeros(H, dtype=np.float32)
    part, _, cls = ref.layernorm_rows(M, H, H)
    if rebuild:
        calls = []
        for c in ref.LN_CLASSES:
            r = rng.normal(0, 1, (M, H))
            if c == "outlier":
                r[np.arange(M), (7 * np.arange(M) + 3) % H] += 40
            mean = 0.0 if c == "ratio0" else 4.0
            sd = {"ratio0": 1.0, "ratio1": 4.0, "ratio4": 1.0, "ratio16": 0.25, "outlier": 1.0, "near-constant": 0.0625}[c]
            calls.append((r.astype(np.float16), np.full(H, sd, dtype=np.float32), np.full(H, mean, dtype=np.float32), zeros, [c] * M))
    else:
        calls = [(part, None, None, np.full(H, 4.0, dtype=np.float32), cls)]
    for r, rg, rb, b1, classes in calls:
        u, out, rows = pybert.test_gemm_lnfold(A1, W1, b1, r, rg, rb, W2, zeros, g, zeros, 0)
        assert np.isfinite(u).all() and np.isfinite(out).all() and np.isfinite(rows).all()
        uf = ref.f8(u)
        mu, sd = uf.mean(axis=1, keepdims=True), np.sqrt(uf.var(axis=1, keepdims=True) + 1e-5)
        ratio = (np.abs(mu) / sd).ravel()
        want = ref.layernorm(uf, ref.f8(g), 0.0)
        bound = ref.layernorm_bound(uf, g, want, one_pass=True) + (2.0 ** -20 * np.abs(mu) + 4 * 9 * ref.U32 * (np.abs(uf) + np.abs(mu))) / sd * ref.f8(g)
        _by_class(out, want, bound, classes, f"fold H {H} rebuild {rebuild} ({classes[0] if rebuild else 'all'}: mean / std up to {ratio.max():.1f})")
        # the row statistics themselves: {1 / std, - mean / std, - mean, std}
        mean_err, rstd_rel = ref.layernorm_stats_bound(uf, one_pass=True)
        assert (np.abs(-ref.f8(rows[:, 2:3]) - mu) <= mean_err + ref.U32 * np.abs(mu)).all()
        assert (np.abs(ref.f8(rows[:, 0:1]) * sd - 1) <= rstd_rel + 4 * ref.U32).all(), float((np.abs(ref.f8(rows[:, 0:1]) * sd - 1) / rstd_rel).max())
        assert (np.abs(ref.f8(rows[:, 3:4]) / sd - 1) <= rstd_rel + 4 * ref.U32).all()


@pytest.mark.parametrize("H", [256, 384])
def test_layernorm_of_the_embedding_kernel(H, M=33):
    """embed_ln (two passes): word rows + the type row (4.0) + small position rows, f32 tables: three f32 terms, two roundings.
    Worst measured fractions of the bound (H = 256 / 384): 0.47 / 0.46 at mean / std 0, 0.44 / 0.42 at 1, 0.27 / 0.26 at 4,
    0.07 / 0.07 at 16, 0.01 / 0.02 near-constant, 0.42 / 0.38 outlier."""
    part, _, cls = ref.layernorm_rows(M, H, 2 * H)
    rng = np.random.default_rng(H)
    g, be = _ln_params(rng, H)
    word = part.astype(np.float32)
    typ = np.full((2, H), 4.0, dtype=np.float32)
    pos = (rng.integers(-8, 9, size=(M, H)) / 1024.0).astype(np.float32)
    got = pybert.test_embed_ln(0, word.view(np.uint8), typ.view(np.uint8), pos.view(np.uint8), H, g, be, np.arange(M, dtype=np.int32),
                               np.array([0, M], dtype=np.int32))
    rows = ref.f8(word) + 4.0 + ref.f8(pos)
    want = ref.layernorm(rows, ref.f8(g), ref.f8(be))
    bound = ref.layernorm_bound(rows, g, want, one_pass=True) + ref.layernorm_input_term(rows, g, 2 * ref.U32 * (np.abs(ref.f8(word)) + 4.0 + np.abs(ref.f8(pos))))
    assert np.isfinite(got).all()
    _by_class(got, want, bound, cls, f"embed_ln H {H}")


@pytest.mark.parametrize("H", [256, 384])
def test_layernorm_of_the_latency_route_s_projection(H, M=33):
    """skinny.hip's LayerNorm-fused Q|K|V projection (device.h layernorm_runs_of and layernorm_scale, the arithmetic of
    layer_tail.hip's LayerNorms): f32 rows in, the normalised f16 rows out.  Worst measured fractions of the bound (H = 256 / 384):
    0.46 / 0.45 at mean / std 0, 0.44 / 0.42 at 1, 0.26 / 0.26 at 4, 0.07 / 0.06 at 16, 0.02 / 0.01 near-constant, 0.40 / 0.36 outlier."""
    _, rows, cls = ref.layernorm_rows(M, H, 3 * H)
    rng = np.random.default_rng(H)
    g, be = _ln_params(rng, H)
    V = rows.astype(np.float32)
    W, bias = _qkv_weights(H)
    _, ln_out = pybert.test_skinny_qkv(W.view(np.uint8), 1, bias, V=V, gamma=g, beta=be)
    want = ref.layernorm(ref.f8(V), ref.f8(g), ref.f8(be))
    assert np.isfinite(ln_out).all()
    _by_class(ln_out, want, ref.layernorm_bound(V, g, want, one_pass=True), cls, f"skinny qkv H {H}")
