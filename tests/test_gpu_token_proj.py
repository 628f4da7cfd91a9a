"""token_proj.hip through bert_hip_test_token_project against float64 within token_proj_reference.py's bound: one token, a ragged wave
block, two waves, a second workgroup; one k-step, a zero-filled k tail, several ring tiles; one, three and eight accumulator blocks."""
import numpy as np
import pytest

from bert_cpp_amd import pybert
import token_proj_reference as tp

pytestmark = pytest.mark.gpu
F16_NAN, F32_NAN, FLAGS = 0x7E00, 0x7FC00000, [(n, h) for n in (False, True) for h in (False, True)]

def _cu(T, step=48):
    return np.array(list(range(0, T, step)) + [T], dtype=np.int32)

def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)

@pytest.mark.parametrize("P", [32, 96, 256])
@pytest.mark.parametrize("H", [16, 40, 384])
@pytest.mark.parametrize("T", [1, 31, 33, 129])
def test_rows_within_the_derived_bound(T, H, P):
    rng = np.random.default_rng(10000 * T + 10 * H + P)
    x = rng.normal(0.1, 1, (T, H)).astype(np.float16)
    wp = rng.normal(0, 1 / np.sqrt(H), (P, H)).astype(np.float16)
    for normalize, f16_out in FLAGS:
        got = pybert.test_token_project(x, wp, _cu(T), 128, normalize, f16_out)
        assert got.dtype == (np.float16 if f16_out else np.float32) and got.shape == (T, P)
        want, bound = tp.project_reference(x, wp, normalize, f16_out)
        err = np.abs(got.astype(np.float64) - want)
        print(f"measured T={T} H={H} P={P} normalize={int(normalize)} f16={int(f16_out)}: worst |got - ref| / bound = {float((err / bound).max()):.3f}")
        assert np.isfinite(bound).all() and (err <= bound).all()
        # NaNs behind row T of x, and in the output beforehand, change no returned bit
        with pybert.test_pad(F16_NAN, F32_NAN):
            assert np.array_equal(_bits(pybert.test_token_project(x, wp, _cu(T), 128, normalize, f16_out)), _bits(got))

@pytest.mark.parametrize("H,P", [(40, 96), (384, 256)])
def test_exact_sums_zero_rows_and_the_norm_order(H, P):
    T = 129
    x, wp = tp.exact_operands(np.random.default_rng(H + P), T, H, P)
    x[[0, 40, 128]] = 0
    v = (x.astype(np.float64) @ wp.astype(np.float64).T).astype(np.float32)          # exact: |sum| < 2^24
    got = pybert.test_token_project(x, wp, _cu(T), 128, False, False)
    assert np.array_equal(_bits(got), _bits(v)) and not got[[0, 40, 128]].any()
    assert np.array_equal(pybert.test_token_project(x, wp, _cu(T), 128, False, True).astype(np.float32), v.astype(np.float16).astype(np.float32))
    # normalised: the float32 restatement of the summation order, bit for bit; a zero row is 0 * inf
    got, want, zero = pybert.test_token_project(x, wp, _cu(T), 128, True, False), tp.normalize_f32(v), ~v.any(axis=1)
    assert zero[[0, 40, 128]].all() and np.isnan(got[zero]).all() and np.isfinite(got[~zero]).all()
    assert np.array_equal(_bits(got[~zero]), _bits(want[~zero]))
    assert np.array_equal(_bits(pybert.test_token_project(x, wp, _cu(T), 128, True, True)[~zero]), _bits(want[~zero].astype(np.float16)))

@pytest.mark.parametrize("f16_out", [False, True])
def test_guard(f16_out):
    rng, cu = np.random.default_rng(7), np.array([0, 5, 5, 75, 100, 100, 131], dtype=np.int32)      # a long sentence, two empty ones
    x, wp = rng.normal(0, 1, (131, 40)).astype(np.float16), rng.normal(0, 0.2, (96, 40)).astype(np.float16)
    free, got = pybert.test_token_project(x, wp, cu, 128, True, f16_out), pybert.test_token_project(x, wp, cu, 64, True, f16_out)
    assert np.isfinite(free).all() and np.isnan(got[5:75]).all()
    keep = np.r_[0:5, 75:131]
    assert np.array_equal(_bits(got[keep]), _bits(free[keep]))
