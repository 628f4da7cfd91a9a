"""The derived error bounds of the f32 route's op-level tests (f32_reference.py; test_gpu_f32_route.py holds the kernels to them on the
GPU) against NumPy float32 emulations of the device arithmetic, on the inputs the GPU tests use -- and against deliberately wrong
emulations, which every bound must refuse.  So the bounds are known to admit the arithmetic they were derived for, and to catch the
breaks they are there to catch, before anything runs on a GPU."""
import numpy as np
import pytest

import f32_reference as f32
import layer_reference as ref
from f32_reference import f4, f8


def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def test_gemm_shapes_cover_what_the_issue_lists():
    Ms, Ns, Ks = ({s[i] for s in f32.GEMM_SHAPES} for i in range(3))
    assert {1, 31, 32, 33, 63, 64, 65, 129} <= Ms and {1, 3, 4, 5, 31, 33, 63, 64, 65, 100, 130} <= Ns
    assert {1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 33, 100, 384} <= Ks
    assert {(1, 1, 1), (65, 65, 17), (33, 130, 100), (129, 100, 33), (130, 1536, 384)} <= set(f32.GEMM_SHAPES)
    assert len(f32.GEMM_SHAPES) == len(set(f32.GEMM_SHAPES)) == 40


@pytest.mark.parametrize("M,N,K", [s for s in f32.GEMM_SHAPES if s[1] <= 130])
def test_matmul_emulations_stay_inside_the_bound(M, N, K):
    """A sequential f32 fma chain and NumPy's pairwise f32 sum of rounded products, bias and bias + residual.  Worst fraction of the
    bound over the shapes: 0.93 at K = 1 (one rounding of the product and one of the sum, both all but half an ulp), 0.69 at K = 2,
    0.13 at K = 17 and less beyond, where the bound is the worst case of K roundings of one sign."""
    A, W, bias, resid = f32.gemm_inputs(M, N, K)
    for r in (None, resid):
        bound, want, _ = f32.matmul_bound(A, W, bias, r)
        for name, got in (("chain", f32.fma_chain(A, W, bias, r)), ("pairwise", f32.matmul_pairwise_f32(A, W, bias, r))):
            err = np.abs(f8(got) - want)
            assert (err <= bound).all(), (name, r is not None, _worst(err, bound))


@pytest.mark.parametrize("M,N,K", [(33, 130, 100), (65, 65, 17), (1, 1, 1), (64, 1, 384), (1, 3, 2)])
def test_matmul_bound_refuses_a_dropped_or_repeated_k(M, N, K):
    """the last k left out (F32_BK / 2 - 1 k-steps on a one-tile K; a partial tile's `hi` lanes reading zeros they should not), and
    k = 2 kk read by both halves of the wave (every odd k replaced by the even one in front of it)"""
    A, W, bias, resid = f32.gemm_inputs(M, N, K)
    bound, want, _ = f32.matmul_bound(A, W, bias, None)
    dropped = f8(A[:, :K - 1]) @ f8(W[:, :K - 1]).T + f8(bias)
    assert (np.abs(dropped - want) > bound).mean() > 0.99
    if K > 1:
        even = np.arange(K) // 2 * 2
        doubled = f8(A[:, even]) @ f8(W[:, even]).T + f8(bias)
        assert (np.abs(doubled - want) > bound).mean() > 0.99


def _gelu_pre(bias):
    x = ref.gelu_sweep()
    x = x[np.abs(f8(x)) >= 2.0 ** -14]           # (normal values: the module's docstring)
    return (x[:, None].astype(np.float32) + ref.gelu_biases(64)[bias][None, :]).astype(np.float32)


@pytest.mark.parametrize("bias", ["zero", "f32"])
def test_gelu_emulation_stays_inside_its_bound_and_another_gelu_does_not(bias):
    """f32 arithmetic with a correctly rounded tanh (half an ulp; the bound allows the device f32.TANHF_ULP).  The bound is absolute in
    the error of 1 + tanh: at x = -5 it is 3.7e-7 (2.5 |x| ulps of a tanh beside -1, 2^-24 each) where gelu itself is -2.3e-7.  Worst
    fraction of the bound: 0.86, at x = 0.0026 (the roundings of the argument).  x sigmoid(1.702 x) is outside it on more than half of
    the sweep, and a kernel that returned 0 below -3 on all of (-4.5, -3)."""
    pre = _gelu_pre(bias)
    pre = pre[np.abs(pre) < 1e18]                # (x^2 finite in f32)
    want, bound = ref.gelu(f8(pre)), f32.gelu_bound(f8(pre), 0.0)
    got = f32.gelu_f32(pre)
    err = np.abs(f8(got) - want)
    assert np.isfinite(got).all() and (err <= bound).all(), (_worst(err, bound), float(pre.ravel()[np.argmax(err / bound)]))
    with np.errstate(over="ignore"):
        sigmoid = f8(pre) / (1 + np.exp(-1.702 * f8(pre)))
    assert (np.abs(sigmoid - want) > bound).mean() > 0.5
    band = (pre < -3) & (pre > -4.5)
    assert band.sum() > 1000 and (np.abs(want[band]) > bound[band]).all()


@pytest.mark.parametrize("n_head,d_head", [(2, 32), (5, 20), (1, 65), (2, 96), (3, 7)])
def test_attention_emulation_stays_inside_its_bound_and_a_missing_scale_does_not(n_head, d_head):
    """Worst fraction of the bound 0.05 - 0.2: it is the worst case of d + n roundings of one sign.  Without 1 / sqrt(d), and with the
    sum of the first 64 numerators only (one key short at n = 65), most elements are outside."""
    lens = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129)
    qkv = f32.attention_inputs(lens, n_head, d_head)
    H, t0 = n_head * d_head, 0
    for n in lens:
        q, k, v = (qkv[t0:t0 + n, i * H:i * H + d_head] for i in range(3))
        t0 += n
        bound, want = f32.softmax_bound(q, k, v)
        assert np.abs(want - f32.attention(q, k, v)).max() < 1e-12
        err = np.abs(f8(f32.attention_f32(q, k, v)) - want)
        assert (err <= bound).all(), (n, _worst(err, bound))
        if n >= 3:
            assert (np.abs(f8(f32.attention_f32(q, k, v, scale=1.0)) - want) > bound).mean() > 0.9, n
        if n > 64:
            sc = f8(q) @ f8(k).T / np.sqrt(d_head)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            assert (np.abs(p @ f8(v) / p[:, :64].sum(axis=1, keepdims=True) - want) > bound).mean() > 0.5, n


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("n", [17, 129])
def test_attention_emulation_on_the_hard_softmax_cases(n, d):
    """layer_reference.SOFTMAX_CASES through the f32 emulation and bound: their f16 values are exact in f32, and normal there (the V
    of subnormal-v too)."""
    for case in ref.SOFTMAX_CASES:
        q, k, v = ref.softmax_case(case, n, d)
        bound, want = f32.softmax_bound(q, k, v)
        err = np.abs(f8(f32.attention_f32(q, k, v)) - want)
        assert (err <= bound).all(), (case, _worst(err, bound))


@pytest.mark.parametrize("H", [1, 7, 63, 64, 65, 100, 384])
def test_two_pass_layernorm_emulation_stays_inside_its_bound(H):
    """f32 two-pass statistics in NumPy's pairwise order on layernorm_rows' classes, mean / std up to 64.  The uncentred second moment
    in place of the variance is outside the bound on every row whose mean is not 0.  (One-pass statistics, E[v^2] - mean^2 in f32,
    are NOT told from two-pass ones by this bound: at H = 384 their emulation reaches 0.52 of it at mean / std 64 and 0.004 at 16 --
    the bound is the worst case of H roundings of one sign in the mean, which grows with mean / std just as the one-pass error does.)"""
    v, g, b, cls = f32.layernorm_inputs(H, 23)
    want = ref.layernorm(f8(v), f8(g), f8(b))
    bound = f32.layernorm_bound(v, g, want)
    err = np.abs(f8(f32.layernorm_two_pass_f32(v, g, b)) - want)
    assert (err <= bound).all(), _worst(err, bound)
    if H > 1:
        mu = f8(v).mean(axis=1, keepdims=True)
        uncentred = (f8(v) - mu) / np.sqrt((f8(v) ** 2).mean(axis=1, keepdims=True) + 1e-5) * f8(g) + f8(b)
        off = [c != "ratio0" for c in cls]
        assert (np.abs(uncentred - want)[off] > bound[off]).mean() > 0.9


@pytest.mark.parametrize("H", [1, 63, 100, 256, 257, 384])
def test_pool_emulation_stays_inside_its_bound(H):
    """All four modes on f32 rows; a norm made of the first two wave sums only is outside the bound wherever a third wave has
    features (H > 128)."""
    rng = np.random.default_rng(H)
    for n in (1, 2, 5, 33):
        rows = f4(rng.normal(0.1, 1, (n, H)))
        for pooling in ("mean", "cls"):
            for normalize in (True, False):
                bound, want = f32.pool_bound(rows, pooling, normalize)
                got = f32.pool_f32(rows, pooling, normalize)
                err = np.abs(f8(got) - want)
                assert (err <= bound).all(), (n, pooling, normalize, _worst(err, bound))
                if (pooling, normalize) == ("cls", False):
                    assert np.array_equal(got, rows[0])
            if H > 128:
                bound, want = f32.pool_bound(rows, pooling, True)
                assert (np.abs(f8(f32.pool_f32(rows, pooling, True, waves=2)) - want) > bound).all(), (n, pooling)
