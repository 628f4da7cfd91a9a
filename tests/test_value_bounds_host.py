"""The derived error bounds of the value-range tests (layer_reference.py; test_gpu_value_ranges.py holds the kernels to them on the
GPU) against NumPy emulations of the device arithmetic, on exactly the inputs the GPU tests use: float16 for gelu_pk16h, float32
one-pass statistics for layernorm_scale, float32 exponentials with P rounded to f16 for softmax_p8.  So the bounds are known to admit
the arithmetic they were derived for -- and to refuse the breaks they are there to catch -- before anything runs on a GPU."""
import numpy as np
import pytest

import layer_reference as ref


@pytest.mark.parametrize("bias", ["zero", "f32"])
def test_gelu_emulation_stays_inside_its_bound(bias):
    """Worst fraction of the bound: 0.977, at -4.027 (t rounds up to 16: the flush, 6.16e-5 against the 2^-14 allowed for it and the relative terms); 0.50
    away from the flush (the rounding of the result).  No NaN or Inf, nothing positive for a negative argument, and x itself wherever float64 rounds to x (but in the
    subnormals, where x / 2 can be a tie that the device's exact 0.5 rounds the other way)."""
    x = ref.gelu_sweep()
    pre = (x[:, None].astype(np.float32) + ref.gelu_biases(64)[bias][None, :]).astype(np.float32)
    got = ref.gelu_pk16h(pre.astype(np.float16))
    want = ref.gelu(ref.f8(pre))
    err, bound = np.abs(ref.f8(got) - want), ref.gelu_bound(pre)
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (float((err / bound).max()), pre[np.unravel_index(np.argmax(err / bound), err.shape)])
    assert (ref.f8(got)[pre < 0] <= 0).all()
    same = ref.gelu_rounds_to_x(pre)
    assert same.sum() > 1000 and np.array_equal(got[same].view(np.uint16), pre.astype(np.float16)[same].view(np.uint16))


def test_gelu_bound_over_every_f16_value_and_what_it_refuses():
    """The emulation on all 63 488 finite f16 values; x sigmoid(1.702 x), the other common approximation, is outside the bound on
    more than 10 000 of them, and a kernel that returned 0 below -3 on every value there down to the flush."""
    x = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    x = x[np.isfinite(x)]
    want, bound = ref.gelu(ref.f8(x)), ref.gelu_bound(x.astype(np.float32))
    assert (np.abs(ref.f8(ref.gelu_pk16h(x)) - want) <= bound).all()
    with np.errstate(over="ignore"):
        sigmoid = (ref.f8(x) / (1 + np.exp(-1.702 * ref.f8(x)))).astype(np.float16)
    assert (np.abs(ref.f8(sigmoid) - want) > bound).sum() > 10000
    band = (ref.f8(x) < -3) & (ref.f8(x) > -4)
    assert (np.abs(want[band]) > bound[band]).all()
    # (where the tolerance of the mat-mul tests has its absolute 4e-3, below -3, the whole bound is under a fiftieth of it)
    assert bound[ref.f8(x) < -3].max() < 4e-3 / 50


@pytest.mark.parametrize("H", [256, 384, 768])
def test_one_pass_layernorm_emulation_stays_inside_its_bound(H):
    """float32 sums in NumPy's pairwise order: 0.47 of the bound at mean / std 0 (the rounding to f16), 0.09 at 16 and 0.01 on the
    near-constant rows, where the bound is the worst case of H roundings of one sign and the sums' errors all but cancel."""
    part, rows, cls = ref.layernorm_rows(33, H, H)
    rng = np.random.default_rng(H)
    g, b = (1 + rng.normal(0, 0.1, H)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    v32 = np.float32(4.0) + part.astype(np.float32)
    want = ref.layernorm(rows, ref.f8(g), ref.f8(b))
    got = ref.layernorm_one_pass(v32, g, b)
    bound = ref.layernorm_bound(rows, g, want, one_pass=True) + ref.layernorm_input_term(rows, g, ref.U32 * np.abs(rows))
    err = np.abs(ref.f8(got) - want)
    assert np.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
    # the classes are what they say
    ratio = np.abs(rows.mean(axis=1)) / rows.std(axis=1)
    for m, c in enumerate(cls):
        lo, hi = {"ratio0": (0, 0.2), "ratio1": (0.8, 1.25), "ratio4": (3.4, 4.7), "ratio16": (14, 18.5), "outlier": (0, 2.5), "near-constant": (55, 75)}[c]
        assert lo <= ratio[m] <= hi, (c, float(ratio[m]))
    assert (np.abs(rows - rows.mean(axis=1, keepdims=True)).max(axis=1)[[c == "outlier" for c in cls]] > 35).all()


def test_one_pass_limit():
    """mean / std at which the one-pass term alone is an f16 ulp of a normalised value of magnitude 1 (DESIGN.md names these)"""
    assert [round(ref.one_pass_limit(H), 1) for H in (256, 384, 768)] == [4.6, 3.7, 2.6]
    v = 3.7 + np.random.default_rng(0).normal(0, 1, (64, 384))
    _, rel = ref.layernorm_stats_bound(v, one_pass=True)
    _, rel2 = ref.layernorm_stats_bound(v)
    assert 0.7 * 2.0 ** -10 < np.median(rel - rel2) < 1.4 * 2.0 ** -10


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("n", ref.SOFTMAX_LENS)
def test_online_softmax_emulation_stays_inside_its_bound(n, d):
    """Worst fractions of the bound: identical 0.21, rising / falling 0.42, wide 0.10, big-v 0.34, subnormal-v 0.48; the ahead-*
    cases are exact (the output is one row of V).  And the cases are what they say."""
    scale = 1 / np.sqrt(d)
    for case in ref.SOFTMAX_CASES:
        q, k, v = ref.softmax_case(case, n, d)
        bound, want = ref.softmax_bound(q, k, v, scale)
        got = ref.softmax_online(q, k, v, scale)
        err = np.abs(ref.f8(got) - want)
        assert np.isfinite(got).all() and (err <= bound).all(), (case, float((err / bound).max()))
        sc = np.sort(ref.f8(q) @ ref.f8(k).T * scale, axis=1)
        if case.startswith("ahead") and n > 1:
            assert (sc[:, -1] - sc[:, -2]).min() >= 40, (case, float((sc[:, -1] - sc[:, -2]).min()))
        if case in ("ahead-per-query", "wide") and n > 128 or case in ("rising", "falling") and n > 384:
            assert 200 < np.abs(sc).max() < 420, (case, float(np.abs(sc).max()))
        if case == "identical":
            assert np.abs(want - ref.f8(v).mean(axis=0)).max() < 1e-12
        if case == "big-v":
            assert 2.0 ** 10 <= np.abs(ref.f8(v)).min() and np.abs(ref.f8(v)).max() <= 2.0 ** 14
        if case == "subnormal-v":
            assert np.abs(ref.f8(v)).max() < 6.1e-5


def test_softmax_bound_refuses_a_missing_rescale():
    """attention.hip's o *= alpha left out: the earlier chunks' numerators keep the scale of their own maximum"""
    n, d = 257, 32
    q, k, v = ref.softmax_case("rising", n, d)
    bound, want = ref.softmax_bound(q, k, v, 1 / np.sqrt(d))
    sc = ref.f8(q) @ ref.f8(k).T / np.sqrt(d)
    o, l, m = np.zeros((n, d)), np.zeros((n, 1)), np.full((n, 1), -np.inf)
    for c in range(0, n, 128):
        m_new = np.maximum(m, sc[:, c:c + 128].max(axis=1, keepdims=True))
        p = np.exp(sc[:, c:c + 128] - m_new)
        l = l * np.exp(m - m_new) + p.sum(axis=1, keepdims=True)
        o = o + p @ ref.f8(v)[c:c + 128]                    # (no o *= alpha)
        m = m_new
    assert (np.abs(o / l - want) > bound).mean() > 0.5


# ------------------------------------------------------------------------------------------------
# the generic kernels (test_gpu_generic_kernels.py holds gemm_naive_kernel and attention_naive_kernel to these bounds on the GPU)
# ------------------------------------------------------------------------------------------------
GENERIC_GEMM_SHAPES = [(1, 1, 1), (3, 7, 5), (5, 100, 100), (33, 136, 64), (4, 64, 33), (130, 65, 130), (257, 300, 20)]


@pytest.mark.parametrize("M,N,K", GENERIC_GEMM_SHAPES)
def test_generic_matmul_emulation_stays_inside_its_bound(M, N, K):
    """One ascending f32 chain, the bias, the epilogue, one rounding to f16: worst fraction of the bound 0.499 under the bias and
    residual epilogues (the rounding to f16 is half the ulp the bound allows for it) and 0.176 under the GELU; a k loop that ends one
    term short is outside it on more than half of the elements of every shape (at least 97 % / 83 % / 96 % of them under the three
    epilogues)."""
    A, W, bias, resid = ref.generic_gemm_inputs(M, N, K)
    W16 = W.astype(np.float16)
    for epi in (0, 1, 2):
        bound, want = ref.generic_gemm_bound(A, W16, bias, resid, epi)
        err = np.abs(ref.f8(ref.generic_gemm(A, W16, bias, resid, epi)) - want)
        assert (err <= bound).all(), (epi, float((err / bound).max()))
        short = np.abs(ref.f8(ref.generic_gemm(A, W16, bias, resid, epi, k_terms=K - 1)) - want)
        assert (short > bound).mean() > 0.5, (epi, float((short > bound).mean()))


@pytest.mark.parametrize("d", [2, 20, 33, 64, 96])
def test_generic_attention_emulation_stays_inside_its_bound(d):
    """The two-pass softmax with exp2(x log2(e)) in float32 on the lengths the GPU test uses: worst fraction of the bound 0.49 (the
    rounding to f16).  With the sum of 63 of the 64 lanes (lane 63's keys 63 and 127 missing from L) every sentence of 64 keys or
    more is outside it, on more than a third of its elements (67 % to 94 %); a shorter one does not use the lane."""
    lens = [1, 2, 3, 4, 5, 63, 64, 65, 130]
    qkv = ref.generic_attention_inputs(tuple(lens), 1, d)
    t0 = 0
    for n in lens:
        q, k, v = (qkv[t0:t0 + n, i * d:(i + 1) * d] for i in range(3))
        t0 += n
        bound, want = ref.generic_attention_bound(q, k, v)
        err = np.abs(ref.f8(ref.generic_attention(q, k, v)) - want)
        assert (err <= bound).all(), (n, float((err / bound).max()))
        short = np.abs(ref.f8(ref.generic_attention(q, k, v, lanes=63)) - want)
        if n >= 64:
            assert (short > bound).mean() > 1 / 3, (n, float((short > bound).mean()))
        else:
            assert (short <= bound).all()


@pytest.mark.parametrize("n", [1, 17, 129])
def test_generic_attention_bound_on_the_hard_softmax_cases(n, d=20):
    """layer_reference.SOFTMAX_CASES through the emulation: scores of +-300 (exponentials flushed to zero), one key 40 ahead, |V| up to
    2^14 and in the subnormals -- all inside the bound (worst 0.498, subnormal-v), nothing NaN; the
    ahead-* cases are exact."""
    for case in ref.SOFTMAX_CASES:
        q, k, v = ref.softmax_case(case, n, d)
        bound, want = ref.generic_attention_bound(q, k, v)
        got = ref.generic_attention(q, k, v)
        err = np.abs(ref.f8(got) - want)
        assert np.isfinite(got).all() and (err <= bound).all(), (case, float((err / bound).max()))


def test_native_expf_bound_admits_the_emulated_exp2():
    """exp2 of the ROUNDED product x log2(e) against exp(x) on [-87, 0]: inside native_expf_rel with one of its two ulps to spare (worst 0.59
    of the whole)"""
    x = -np.random.default_rng(0).uniform(0, 87, 100000).astype(np.float32)
    got = np.exp2(ref.f8(x * np.float32(1.44269504088896340736))).astype(np.float32)
    rel = np.abs(ref.f8(got) / np.exp(ref.f8(x)) - 1)
    assert (rel <= ref.native_expf_rel(x) - 2 * ref.U32).all(), float((rel / ref.native_expf_rel(x)).max())
