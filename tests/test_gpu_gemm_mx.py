"""The MXFP8 mat-mul of the forward route on its own (gemm_mx.hip through bert_hip_test_gemm_mx: row quantiser, then the kernel in both
output forms) at the shapes where it can go wrong: one, two and twelve MFMA steps of k (a half-filled, one and six reduction tiles), one
and three feature tiles, one token tile and two with a ragged edge.
The f16 form is held to float64 over the DECODED operands:  |C - ref| <= TOL sum_k |a_k w_k| g + 2^-11 |ref| + 2^-24, g = 1.13 for GELU.
Measured on an MI355X over these very cases (profiles/mx_rate.txt): the largest |C - ref| / sum_k |a_k w_k| is 1.63e-2 (M = 1, K = 64 with
the residual: the f16 rounding of an output whose bias and residual dwarf its 64 products — what the bound's second term is for); the
largest (|C - ref| - 2^-11 |ref| - 2^-24) / (g sum_k |a_k w_k|), what the first term has to carry, is 1.44e-4 (M = 257, K = 64).  TOL is
twice the SMALLER figure: every result that passes under it passes under twice the larger one."""
import numpy as np
import pytest

from bert_cpp_amd import pybert
from mxfp4_reference import mxfp8_queries

pytestmark = pytest.mark.gpu
MEASURED = 1.44e-4
TOL = 2 * MEASURED


def operands(M, N, K):
    rng = np.random.default_rng(1000 * M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float16)
    A[0, 0:32] = 0                                            # a zero block
    A[M - 1, K - 32:K] *= np.float16(0.01)                    # an outlier block: one value 5000 times its neighbours
    A[M - 1, K - 7] = np.float16(50)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float16)
    return A, W, rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float16)


def gelu(x):
    return 0.5 * x * (1 + np.tanh(0.7978845608028654 * x * (1 + 0.044715 * x * x)))


@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("N,K", [(128, 64), (384, 128), (128, 768)])
@pytest.mark.parametrize("M", [1, 255, 257])
def test_both_output_forms(M, N, K, epi):
    A, W, bias, resid = operands(M, N, K)
    resid = resid if epi == 2 else None
    C, (cq, cs), (aq, asc) = pybert.test_gemm_mx(A, W, bias, resid, epi)
    # operands: the quantiser's rows are the reference rule's, bit for bit (signs of zeros aside: a code 0x80 is -0)
    a = pybert.mx_decode(aq, asc)
    assert np.array_equal(a.view(np.int32) & 0x7fffffff, mxfp8_queries(A.astype(np.float32)).view(np.int32) & 0x7fffffff)
    assert np.array_equal(aq >> 7, np.signbit(A).astype(np.uint8))
    # the f16 form against float64 over the decoded operands
    w = pybert.mx_decode(*pybert.test_pack_mx(W)).astype(np.float64)
    a = a.astype(np.float64)
    ref, mass = a @ w.T + bias, np.abs(a) @ np.abs(w).T
    ref = gelu(ref) if epi == 1 else ref + resid if epi == 2 else ref
    err = np.abs(C.astype(np.float64) - ref)
    g, rounding = (1.13 if epi == 1 else 1.0), 2.0 ** -11 * np.abs(ref) + 2.0 ** -24
    print(f"measured M={M} N={N} K={K} epi={epi}: worst |C - ref| / mass = {float((err / mass).max()):.3e}, beyond the rounding {float(((err - rounding) / (g * mass)).max()):.3e}")
    assert (err <= TOL * mass * g + rounding).all()
    # the MX form: the row quantiser on the f16 form's own output, fused
    c = pybert.mx_decode(cq, cs)
    assert np.array_equal(c.view(np.int32) & 0x7fffffff, mxfp8_queries(C.astype(np.float32)).view(np.int32) & 0x7fffffff)
    assert np.array_equal(cq >> 7, np.signbit(C).astype(np.uint8))
    # padding: NaNs behind the last token, in every input and in every buffer before the first launch, change no returned bit
    with pybert.test_pad(0x7E00, 0x7FC00000):
        C2, (cq2, cs2), (aq2, asc2) = pybert.test_gemm_mx(A, W, bias, resid, epi)
    for got, want in ((C2.view(np.uint16), C.view(np.uint16)), (cq2, cq), (cs2, cs), (aq2, aq), (asc2, asc)):
        assert np.array_equal(got, want)
