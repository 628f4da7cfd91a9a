"""The host side of the weight packing (csrc/weights.cpp), bit for bit, without a GPU.

The expectations are a NumPy restatement of the layout comments of kernels.h (GemmWeight, GemmLnFold) and weights.h, not of the C++:
every form the engine uploads is rebuilt here from the file bytes and compared byte by byte with bert_hip_test_pack_weight.
This is deterministic host arithmetic, so there is no tolerance anywhere."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

F32, F16, Q4_0, Q4_1 = 0, 1, 2, 3
WTYPES = [F32, F16, Q4_0, Q4_1]
# (N, K, three stacked tensors): N not a multiple of the 128-row tile (200, 72, 264), the smallest K of the MFMA kernels and
# bert-base's largest, and a stacked Q | K | V triple whose parts (88 rows) end inside a tile
SHAPES = [(200, 64, False), (72, 3072, False), (264, 128, True), (256, 64, False)]
K16_ORDER = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def file_bytes(w: np.ndarray, wtype: int) -> np.ndarray:
    """f32 [N][K] -> the tensor as a model file stores it"""
    if wtype == F32:
        return w.astype(np.float32).view(np.uint8).reshape(-1)
    if wtype == F16:
        return w.astype(np.float16).view(np.uint8).reshape(-1)
    return (gf.quantize_q4_0 if wtype == Q4_0 else gf.quantize_q4_1)(w).reshape(-1)


def q4_blocks(raw: np.ndarray, wtype: int, N: int, K: int):
    """file bytes -> d, m as f16 [N][K/32] (m = 0 for q4_0) and the 4-bit values [N][K/32][32] in element order: byte j of a
    block holds elements j (low nibble) and j + 16 (high nibble)"""
    hdr = 2 if wtype == Q4_0 else 4
    blk = raw.reshape(N, K // 32, hdr + 16)
    d = blk[:, :, 0:2].copy().view(np.float16)[:, :, 0]
    m = blk[:, :, 2:4].copy().view(np.float16)[:, :, 0] if wtype == Q4_1 else np.zeros_like(d)
    qs = blk[:, :, hdr:]
    return d, m, np.concatenate([qs & 0x0F, qs >> 4], axis=2)


def rows_f16(raw: np.ndarray, wtype: int, N: int, K: int) -> np.ndarray:
    """the f16 value of every weight: f16 files as stored, f32 files rounded once, q4_0 (q - 8) d (exact in f32) rounded once,
    q4_1 q d + m computed exactly (float64) and rounded ONCE to f16"""
    if wtype == F32:
        return raw.view(np.float32).reshape(N, K).astype(np.float16)
    if wtype == F16:
        return raw.view(np.float16).reshape(N, K).copy()
    d, m, q = q4_blocks(raw, wtype, N, K)
    if wtype == Q4_0:
        v = (q.astype(np.float32) - np.float32(8)) * d.astype(np.float32)[:, :, None]
    else:
        v = q.astype(np.float64) * d.astype(np.float64)[:, :, None] + m.astype(np.float64)[:, :, None]
    return v.astype(np.float16).reshape(N, K)


def table_f32(raw: np.ndarray, wtype: int, N: int, K: int) -> np.ndarray:
    """an embedding table of a q4 file: (q - 8) d, or q d + m, in f32 arithmetic (what the gather kernel computes)"""
    d, m, q = q4_blocks(raw, wtype, N, K)
    d32, m32, q32 = d.astype(np.float32)[:, :, None], m.astype(np.float32)[:, :, None], q.astype(np.float32)
    v = (q32 - np.float32(8)) * d32 if wtype == Q4_0 else q32 * d32 + m32
    assert v.dtype == np.float32
    return v.reshape(N, K)


def padded(rows: np.ndarray) -> np.ndarray:
    N, K = rows.shape
    img = np.zeros(((N + 127) // 128 * 128, K), dtype=rows.dtype)
    img[:N] = rows
    return img


def ln_fold(rows: np.ndarray, gamma, beta, bias):
    """image = f16(W gamma) (product in f32); columns s_hi s_lo s_hi c_hi c_lo c_hi 0 ... with s = sum_k W'[n][k] and
    c = bias[n] + sum_k beta[k] W[n][k], both summed in float64 in index order (cumsum is sequential, sum is not)"""
    N, K = rows.shape
    w32 = rows.astype(np.float32)
    folded = (w32 * gamma[None, :]).astype(np.float16)
    s = np.cumsum(folded.astype(np.float64), axis=1)[:, -1]
    start = np.zeros(N) if bias is None else bias.astype(np.float64)
    c = np.cumsum(np.concatenate([start[:, None], beta.astype(np.float64)[None, :] * w32.astype(np.float64)], axis=1), axis=1)[:, -1]
    aug = np.zeros((N, 16), dtype=np.float16)
    for col, v in ((0, s), (3, c)):
        hi = v.astype(np.float32).astype(np.float16)
        lo = (v - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
        aug[:, col], aug[:, col + 1], aug[:, col + 2] = hi, lo, hi
    return padded(folded), aug


def make(N: int, K: int, wtype: int, seed: int):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    return file_bytes(w, wtype), rng


def same(got: np.ndarray, want: np.ndarray):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.nbytes == want.nbytes, (got.nbytes, want.nbytes)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}"


@pytest.mark.parametrize("wtype", WTYPES, ids=["f32", "f16", "q4_0", "q4_1"])
@pytest.mark.parametrize("N,K,stack3", SHAPES)
def test_f16_images(N, K, stack3, wtype):
    raw, _ = make(N, K, wtype, seed=N + K + wtype)
    img = padded(rows_f16(raw, wtype, N, K))
    assert N % 128 == 0 or not img[N:].any()
    same(pybert.pack_weight(raw, wtype, N, K, "f16", stack3=stack3), img)
    # the k order [0-3, 8-11, 4-7, 12-15] inside every group of 16
    same(pybert.pack_weight(raw, wtype, N, K, "f16_kperm", stack3=stack3), img.reshape(-1, 16)[:, K16_ORDER])


@pytest.mark.parametrize("wtype", [Q4_0, Q4_1], ids=["q4_0", "q4_1"])
@pytest.mark.parametrize("N,K,stack3", SHAPES)
def test_q4_planes(N, K, stack3, wtype):
    raw, _ = make(N, K, wtype, seed=N + K + wtype)
    hdr = 2 if wtype == Q4_0 else 4
    blk = raw.reshape(N, K // 32, hdr + 16)
    n, b = np.meshgrid(np.arange(N), np.arange(K // 32), indexing="ij")
    # one 16-byte unit of nibbles and one scale entry per 32-weight block at ((nt (K/64) + kt) 128 + row) 2 + block
    index = (((n // 128) * (K // 64) + b // 2) * 128 + n % 128) * 2 + b % 2
    n_blocks = (N + 127) // 128 * (K // 64) * 256
    qs = np.zeros((n_blocks, 16), dtype=np.uint8)
    sc = np.zeros((n_blocks, hdr), dtype=np.uint8)
    qs[index] = blk[:, :, hdr:]
    sc[index] = blk[:, :, :hdr]
    same(pybert.pack_weight(raw, wtype, N, K, "q4_nibbles", stack3=stack3), qs)
    same(pybert.pack_weight(raw, wtype, N, K, "q4_scales", stack3=stack3), sc)


@pytest.mark.parametrize("wtype", WTYPES, ids=["f32", "f16", "q4_0", "q4_1"])
@pytest.mark.parametrize("N,K,stack3", SHAPES)
def test_ln_fold_image_and_statistics(N, K, stack3, wtype):
    raw, rng = make(N, K, wtype, seed=N + K + wtype)
    gamma = (1 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    rows = rows_f16(raw, wtype, N, K)
    for b in (bias, None):
        img, aug = ln_fold(rows, gamma, beta, b)
        same(pybert.pack_weight(raw, wtype, N, K, "ln_fold", gamma, beta, b, stack3=stack3), img)
        same(pybert.pack_weight(raw, wtype, N, K, "ln_fold_stats", gamma, beta, b, stack3=stack3), aug)
        assert aug[:, 1].any() and aug[:, 4].any() and not aug[:, 6:].any()      # (the low halves carry something)


def test_gamma_beta_bias_words():
    rng = np.random.default_rng(5)
    gamma, beta, bias = ((rng.standard_normal(768) * s).astype(np.float32) for s in (1.0, 0.3, 0.3))
    g = gamma.astype(np.float16).view(np.uint16).astype(np.uint32)
    bb = (beta + bias).astype(np.float16).view(np.uint16).astype(np.uint32)
    same(pybert.pack_weight(np.zeros(1, dtype=np.uint8), F32, 768, 0, "gamma_beta_bias", gamma, beta, bias), g | (bb << 16))


def blocks_with_a_tiny_minimum(N: int, K: int, seed: int) -> np.ndarray:
    """Blocks whose minimum is f16's smallest subnormal (2^-24) under a scale between 1 and 2.  q d has up to 15 significant bits, so
    it can be the exact middle of two f16 values; q d + m then lies just above that middle.  Rounded once it goes up.  In f32 the
    2^-24 is below the last place: the sum rounds back to the middle, and the tie goes to the even f16, down as often as up."""
    rng = np.random.default_rng(seed)
    nb = N * K // 32
    span = 15 * rng.uniform(1, 2, size=(nb, 1)).astype(np.float32)
    u = rng.random((nb, 32), dtype=np.float32)
    u[:, 0], u[:, 1] = 0, 1                                   # (the block's range is exactly [2^-24, 2^-24 + span])
    return (np.float32(2.0 ** -24) + span * u).astype(np.float32).reshape(N, K)


@pytest.mark.parametrize("wtype", [Q4_0, Q4_1], ids=["q4_0", "q4_1"])
def test_q4_table_as_f32_and_where_it_differs_from_the_f16_image(wtype):
    N, K = 64, 3072
    raw = file_bytes(blocks_with_a_tiny_minimum(N, K, seed=11), wtype)
    table, rows = table_f32(raw, wtype, N, K), rows_f16(raw, wtype, N, K)
    # the two dequantisations differ ON PURPOSE for q4_1 (f32 multiply-add for the gather kernel, one rounding of the exact value
    # for the mat-mul images); this input is the case where it shows: rounding the f32 table to f16 is not the f16 image
    differ = int((table.astype(np.float16) != rows).sum())
    print(f"q4 type {wtype}: {differ} of {N * K} weights differ between f16(f32 table) and the f16 image")
    assert (differ > 0) == (wtype == Q4_1), differ
    same(pybert.pack_weight(raw, wtype, N, K, "table_f32"), table)
    same(pybert.pack_weight(raw, wtype, N, K, "f16"), padded(rows))


@pytest.mark.parametrize("wtype", [Q4_0, Q4_1], ids=["q4_0", "q4_1"])
def test_q4_table_of_ordinary_weights(wtype):
    raw, _ = make(100, 384, wtype, seed=3)
    same(pybert.pack_weight(raw, wtype, 100, 384, "table_f32"), table_f32(raw, wtype, 100, 384))


def test_requests_that_make_no_sense_are_refused():
    raw, _ = make(128, 64, F16, seed=1)
    for form in ("q4_nibbles", "q4_scales", "table_f32", "ln_fold"):      # (planes and tables of an f16 tensor; a fold without gamma)
        with pytest.raises(RuntimeError):
            pybert.pack_weight(raw, F16, 128, 64, form)
    q, _ = make(4, 96, Q4_0, seed=1)
    with pytest.raises(RuntimeError):                                      # (K = 96 and N = 4: not a shape the plane layout holds)
        pybert.pack_weight(q, Q4_0, 4, 96, "q4_nibbles")
