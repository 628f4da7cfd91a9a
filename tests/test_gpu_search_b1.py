"""The 1-bit embedding index (bert_hip_index_create dtype 3, "b1": search.hip's index_pack_b1_kernel and
index_topk_kernel<b1_t>) against a NumPy restatement of its arithmetic: a row keeps bit_i = (x_i > 0); a query is quantized
in float32 like the int8 form's, scale = amax / 127 and code = clamp(rint(x / scale), -127, 127); score = (float)dot * qscale
over the exact integer dot = sum_i code_i * (bit_i ? +1 : -1).  Every check is bit-exact: the same ids, and the same score
bits.  Ties are common with this form, so the (score, id) order rule is exercised by every case.

Recall of the exact top-10 among the best 10 / 100 / 400 candidates of this restatement, unit Gaussian rows (no structure:
the worst case), 2 x 10^5 rows, dim 384, 200 queries: 0.17 / 0.51 / 0.76 (the int8 form's own recall@10 there: 0.98).
Measured in NumPy with the functions below; nothing here is gated on it."""
import ctypes as C
import os

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = os.path.join(ROOT, "tests", "golden", "sample_client_texts_600.txt")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


class _Hip:
    """Just enough of the HIP runtime through ctypes (the runtime libbert.so itself is linked against)."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        assert self.lib.hipMemcpy(C.c_void_p(p), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0
        return p

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def stream(self):
        s = C.c_void_p()
        assert self.lib.hipStreamCreate(C.byref(s)) == 0
        return s.value

    def free(self, *ps):
        for p in ps:
            self.lib.hipFree(C.c_void_p(p))

    def free_bytes(self):
        free, total = C.c_size_t(), C.c_size_t()
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value


# ---- the restatement

def quantize(x):
    """x [n, dim] -> (codes int8 [n, dim], scales float32 [n]): the int8 form's quantizer"""
    x = np.asarray(x, dtype=np.float32)
    finite = np.isfinite(x).all(axis=1)
    amax = np.abs(np.where(np.isfinite(x), x, np.float32(0))).max(axis=1, initial=np.float32(0)).astype(np.float32)
    scale = np.where(finite, amax / np.float32(127), np.float32(np.nan)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.rint(x / scale[:, None])
    keep = (finite & (scale != 0))[:, None]
    return np.where(keep, np.clip(np.where(keep, q, 0), -127, 127), 0).astype(np.int8), scale


def scores(queries, rows):
    qc, qs = quantize(queries)
    with np.errstate(invalid="ignore"):
        bits = np.asarray(rows, dtype=np.float32) > 0                # (IEEE: false for -0, NaN, -inf; true for +inf)
    # |dot| <= 127 * 2048: exact in float64, and in the float32 it is converted to
    dot = qc.astype(np.float64) @ np.where(bits, 1.0, -1.0).T
    with np.errstate(invalid="ignore"):
        return dot.astype(np.float32) * qs[:, None]


def ref_topk(S, k):
    """larger score first, equal scores by smaller id, NaN never returned, -1 / -inf beyond"""
    Q, N = S.shape
    ids = np.full((Q, k), -1, np.int32)
    sc = np.full((Q, k), -np.inf, np.float32)
    for i in range(Q):
        s = S[i]
        valid = np.nonzero(~np.isnan(s))[0]
        n = min(k, len(valid))
        if n == 0:
            continue
        v = s[valid]
        kth = np.partition(v, len(v) - n)[len(v) - n]
        cand = valid[v >= kth]
        order = np.lexsort((cand, -s[cand]))[:n]
        ids[i, :n] = cand[order]
        sc[i, :n] = s[cand[order]]
    return ids, sc


def assert_same(got, want, what=""):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[0]][:8], wi[bad[0]][:8], gs[bad[0]][:8], ws[bad[0]][:8])


def assert_exact(got, rows, queries, k, keep=None, what=""):
    S = scores(queries, rows) if len(rows) else np.zeros((len(queries), 0), np.float32)
    if keep is not None:
        S[:, ~keep] = np.nan                                         # (a NaN score is never returned)
    assert_same(got, ref_topk(S, k), what)


# ---- 1. the grid

def _combos():
    # (N, Q, k) per dim: every N of 0, 1, 127, 128, 129, 1000, 4500 (two slices at k <= 128: a slice holds at least
    # max(2048, 16 k) rows) and 9000 (two slices at k = 256), every Q of 1, 31, 32, 33, 100 and every k of 1, 10, 256 appear,
    # each k with small and large dims
    per_dim = {
        1: [(0, 1, 10), (127, 31, 256), (1000, 100, 1)],
        31: [(1, 32, 1), (128, 33, 10), (4500, 1, 256)],
        32: [(129, 100, 256), (4500, 31, 10), (0, 33, 1)],
        33: [(1000, 32, 10), (1, 1, 256), (127, 100, 1)],
        127: [(128, 1, 1), (9000, 33, 256), (129, 31, 10)],
        128: [(4500, 32, 1), (127, 1, 10), (1000, 33, 256)],
        129: [(1, 100, 10), (129, 32, 256), (4500, 33, 1)],
        384: [(1000, 1, 10), (4500, 100, 10), (128, 31, 1), (9000, 1, 256)],
        2048: [(127, 33, 10), (4500, 1, 1), (1000, 32, 256)],
    }
    for d, cases in per_dim.items():
        for N, Q, k in cases:
            yield d, N, Q, k


@pytest.mark.parametrize("dim,N,Q,k", list(_combos()))
def test_b1_search_grid(model, dim, N, Q, k):
    rng = np.random.default_rng(dim * 1000003 + N * 7 + Q * 3 + k)
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype="b1")
    if N:
        assert ix.add(rows) == 0
    assert len(ix) == N
    assert_exact(ix.search(queries, k), rows, queries, k)
    ix.close()


# ---- 2. special rows and queries, ties

def test_b1_special_elements_follow_x_gt_0(model):
    rng = np.random.default_rng(5)
    dim = 96
    rows = unit_rows(rng, 400, dim)
    rows[3, :] = -0.0
    rows[4, :] = 0.0
    rows[5, ::2] = np.nan
    rows[6, :] = np.nan
    rows[7, :] = np.inf
    rows[8, :] = -np.inf
    rows[9, 1::3] = -np.inf
    rows[10, 5] = np.inf
    rows[11] = np.float32(2.0 ** -140)                               # a positive subnormal is > 0
    rows[12] = -np.float32(2.0 ** -140)
    q = np.concatenate([unit_rows(rng, 30, dim), np.ones((1, dim), np.float32), np.zeros((1, dim), np.float32),
                        np.full((1, dim), np.nan, np.float32), np.zeros((1, dim), np.float32)])
    q[-1, 3] = np.inf
    ix = model.index(dim=dim, dtype="b1")
    ix.add(rows)
    for k in (1, 10, 256):
        assert_exact(ix.search(q, k), rows, q, k, what=k)
    ids, sc = ix.search(q[-4:], 10)
    # an all-ones query: the all-ones rows first (+inf row 7, subnormal row 11), at dot = 127 dim
    assert ids[0, :2].tolist() == [7, 11] and sc[0, 0] == np.float32(127 * dim) * (np.float32(1) / np.float32(127))
    # a zero query: score +0 against every row, the smallest ids win; a NaN or inf query: nothing
    assert ids[1].tolist() == list(range(10)) and (sc[1].view(np.int32) == 0).all()
    assert (ids[2:] == -1).all() and np.isneginf(sc[2:]).all()
    ix.close()


def test_b1_identical_rows_only_the_id_decides(model):
    rng = np.random.default_rng(6)
    dim, N = 200, 700
    x = unit_rows(rng, 1, dim)
    rows = np.repeat(x, N, axis=0) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)     # the same signs in every row
    q = np.concatenate([x, -x, unit_rows(rng, 3, dim)])
    ix = model.index(dim=dim, dtype="b1")
    ix.add(rows)
    for k in (1, 10, 256):
        ids, sc = ix.search(q, k)
        assert (ids == np.arange(k)[None, :]).all()
        assert (sc.view(np.int32) == sc.view(np.int32)[:, :1]).all()
        assert_exact((ids, sc), rows, q, k)
    ix.close()


def test_b1_errors(model):
    ix = model.index(dim=8, dtype="b1")
    ix.add(np.ones((3, 8), np.float32))
    ids, sc = ix.search(np.ones((1, 8), np.float32), 5)              # fewer rows than k
    assert ids[0].tolist() == [0, 1, 2, -1, -1] and np.isneginf(sc[0, 3:]).all()
    for bad in (0, 257):
        with pytest.raises(RuntimeError):
            ix.search(np.ones((1, 8), np.float32), bad)
    ix.close()


# ---- 3. invariance

def test_b1_bitwise_invariance(model):
    rng = np.random.default_rng(9)
    N, dim, Q = 4500, 200, 100
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype="b1")
    ix.add(rows)
    ids, sc = ix.search(queries, 100)
    assert_exact((ids, sc), rows, queries, 100)
    for i in (0, 1, 57, 99):                                         # a query alone
        assert_same(ix.search(queries[i:i + 1], 100), (ids[i:i + 1], sc[i:i + 1]), i)
    assert_same(ix.search(queries, 10), (ids[:, :10], sc[:, :10]), "top-10 is a prefix of top-100")
    # several adds into reserved storage against one add into grown storage
    cuts = np.sort(rng.choice(np.arange(1, N), 12, replace=False))
    parts = model.index(dim=dim, dtype="b1")
    parts.reserve(N, Q, 100)
    for p in np.split(rows, cuts):
        parts.add(p)
    assert len(parts) == N
    assert_same(parts.search(queries, 100), (ids, sc), "parts")
    # the device entry points
    hip = _Hip()
    s = hip.stream()
    d_q, d_i, d_s, d_r = hip.upload(queries), hip.malloc(Q * 100 * 4), hip.malloc(Q * 100 * 4), hip.upload(rows)
    ix.search_device(Q, d_q, 100, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, 100), np.int32), hip.download(d_s, (Q, 100))), (ids, sc), "search_device")
    dev = model.index(dim=dim, dtype="b1")
    assert dev.add_device(N, d_r, s) == 0
    dev.search_device(Q, d_q, 100, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, 100), np.int32), hip.download(d_s, (Q, 100))), (ids, sc), "add_device")
    hip.free(d_q, d_i, d_s, d_r)
    for i in (ix, parts, dev):
        i.close()


# ---- 4. allow-lists, removals, compaction

@pytest.mark.parametrize("dim,N,Q,k", [(7, 129, 33, 10), (384, 4500, 33, 10), (200, 4500, 1, 256), (33, 1000, 100, 1)])
def test_b1_filtered_removed_and_compacted(model, dim, N, Q, k):
    rng = np.random.default_rng(dim + N + Q + k)
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    keep = rng.random(N) < 0.5
    keep[N // 8 * 2:N // 8 * 3] = False                              # whole words without a qualifying row
    ix = model.index(dim=dim, dtype="b1")
    ix.add(rows)
    assert_exact(ix.search(queries, k, allow=keep), rows, queries, k, keep, "allow")
    assert_exact(ix.search(queries, k, allow=np.zeros(N, bool)), rows, queries, k, np.zeros(N, bool), "nothing allowed")
    gone = np.nonzero(~keep)[0]
    assert ix.remove(gone) == len(gone) and ix.n_live == int(keep.sum())
    assert_exact(ix.search(queries, k), rows, queries, k, keep, "removed")
    allow = rng.random(N) < 0.5
    assert_exact(ix.search(queries, k, allow=allow), rows, queries, k, keep & allow, "removed and allowed")
    # compaction: the restatement over the qualifying rows, the new ids mapped back
    before = ix.search(queries, k)
    old = ix.compact()
    assert old.tolist() == np.nonzero(keep)[0].tolist() and len(ix) == int(keep.sum()) == ix.n_live
    post_i, post_s = ix.search(queries, k)
    assert_exact((post_i, post_s), rows[keep], queries, k, what="compacted")
    assert_same((np.where(post_i >= 0, old[np.maximum(post_i, 0)], -1).astype(np.int32), post_s), before, "compacted, ids mapped back")
    # rows added behind a compaction go on from the new size
    extra = unit_rows(rng, 3, dim)
    assert ix.add(extra) == len(old)
    assert_exact(ix.search(queries, k), np.concatenate([rows[keep], extra]), queries, k, what="added after compaction")
    ix.close()


def test_b1_filtered_device_entry(model):
    rng = np.random.default_rng(12)
    N, dim, Q, k = 4500, 64, 33, 10
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    live, allow = rng.random(N) < 0.7, rng.random(N) < 0.5
    hip = _Hip()
    s = hip.stream()
    ix = model.index(dim=dim, dtype="b1")
    ix.reserve(N, Q, k)
    ix.add(rows)
    ix.remove(np.nonzero(~live)[0])
    words = pybert.allow_words(allow, N)
    d_q, d_w, d_i, d_s = hip.upload(q), hip.upload(words), hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
    before = hip.free_bytes()
    ix.search_device(Q, d_q, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words))
    assert hip.free_bytes() == before                                # within reserve's bounds: no allocation
    assert_exact((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), rows, q, k, live & allow)
    hip.free(d_q, d_w, d_i, d_s)
    ix.close()


# ---- 5. files

@pytest.mark.parametrize("dim,N,removed", [(384, 1000, False), (7, 333, True), (129, 0, False)])
def test_b1_save_and_load(model, tmp_path, dim, N, removed):
    rng = np.random.default_rng(dim + N)
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, 9, dim)
    ix = model.index(dim=dim, dtype="b1")
    if N:
        ix.add(rows)
    keep = np.ones(N, bool)
    if removed:
        keep[rng.choice(N, 40, replace=False)] = False
        ix.remove(np.nonzero(~keep)[0])
    path = str(tmp_path / "b1.idx")
    ix.save(path)
    dpad = (dim + 127) // 128 * 128
    assert os.path.getsize(path) == 64 + N * dpad // 8 + ((N + 31) // 32 * 4 if removed else 0)
    if N and not removed:
        # the stored form: bit i & 31 of little-endian u32 word i >> 5 = (x_i > 0), the padding zero
        stored = np.fromfile(path, dtype="<u4", offset=64).reshape(N, dpad // 32)
        bits = ((stored[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(N, dpad).astype(bool)
        assert np.array_equal(bits[:, :dim], rows > 0) and not bits[:, dim:].any()
    back = model.load_index(path)
    assert (back.dtype, back.dim, len(back), back.n_live) == ("b1", dim, N, int(keep.sum()))
    for k in (1, 10):
        want = ix.search(q, k)
        assert_same(back.search(q, k), want, "loaded")
        assert_exact(want, rows, q, k, keep if removed else None)
    back.close()
    ix.close()


# ---- 6. texts, memory, profiler names

def test_b1_text_routes(model):
    with open(TEXTS, encoding="utf-8") as f:
        texts = [line.rstrip("\n") for line in f][:150]
    emb = model.encode_batch(texts)
    a = model.index(dtype="b1")
    assert a.add_texts(texts) == 0
    b = model.index(dtype="b1")
    b.add(emb)
    got = a.search(emb, 20)
    assert_same(got, b.search(emb, 20), "add_texts against encode + add")
    assert_exact(got, emb, emb, 20)
    queries = ["Should I get health insurance?", "poaching", texts[7], texts[123]]
    assert_same(a.search_texts(queries, 5), a.search(model.encode_batch(queries), 5), "search_texts against encode + search")
    a.close()
    b.close()


def test_b1_memory_per_row(model):
    hip = _Hip()
    ix = model.index(dim=384, dtype="b1")
    before = hip.free_bytes()
    ix.reserve(2_000_000, 1, 1)
    used = before - hip.free_bytes()
    ix.close()
    assert 2_000_000 * 48 <= used <= 2_000_000 * 48 + (16 << 20), used     # dpad / 8 = 48 bytes per row


def test_b1_profile_names(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    rng = np.random.default_rng(2)
    ix = m.index(dim=64, dtype="b1")
    ix.add(unit_rows(rng, 5000, 64))
    ix.search(unit_rows(rng, 3, 64), 10)
    ix.remove([1])
    ix.search(unit_rows(rng, 3, 64), 10)
    rep = m.profile_report()
    for name in ("index_pack_b1", "index_quantize_i8", "index_topk_b1", "index_topk_b1_masked"):
        assert name in rep and rep[name]["launches"] >= 1, (name, sorted(rep))
    m.close()
