"""The int8 embedding index (bert_hip_index_create dtype 2: search.hip's index_quantize_kernel and index_topk_kernel<int8_t>)
against a NumPy restatement of its arithmetic: per row and per query, in float32, scale = amax / 127 and
code = clamp(rint(x / scale), -127, 127); score = ((float)dot * qscale) * rscale over an exact integer dot.  Every check is
bit-exact: the same ids, and the same score bits."""
import ctypes as C
import os
import subprocess

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
    """x [n, dim] -> (codes int8 [n, dim], scales float32 [n])"""
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
    rc, rs = quantize(rows)
    # codes are at most 127 in size and dim <= 2048: every partial sum is an integer below 2^53, exact in float64
    dot = qc.astype(np.float64) @ rc.astype(np.float64).T
    with np.errstate(invalid="ignore", over="ignore"):
        return (dot.astype(np.int64).astype(np.float32) * qs[:, None]) * rs[None, :]


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


def assert_exact(ids, sc, rows, queries, k):
    want_i, want_s = ref_topk(scores(queries, rows) if len(rows) else np.zeros((len(queries), 0), np.float32), k)
    assert ids.shape == want_i.shape
    bad = np.nonzero((ids != want_i).any(axis=1) | (sc.view(np.int32) != want_s.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], ids[bad[0]][:8], want_i[bad[0]][:8], sc[bad[0]][:8], want_s[bad[0]][:8])


# ---- 1. the grid

def _combos():
    per_dim = {                     # (N, Q, k): every k with small and large dims, N < k, N not a multiple of 128, Q = 4097
        1: [(0, 3, 10), (31, 64, 256), (1000, 1, 1)],
        31: [(1, 1, 10), (1000, 1000, 100), (65537, 3, 256)],
        32: [(31, 3, 1), (65537, 64, 10), (1000, 1000, 256)],
        33: [(300, 4097, 10), (1000, 64, 100), (65537, 1, 1)],
        200: [(1, 64, 256), (31, 1000, 10), (65537, 100, 100)],
        384: [(1000, 3, 10), (65537, 64, 1), (31, 1, 100)],
        768: [(0, 64, 256), (1000, 1, 100), (65537, 3, 10)],
        2048: [(31, 3, 256), (1000, 64, 10), (65537, 1, 100)],
    }
    for d, cases in per_dim.items():
        for N, Q, k in cases:
            yield d, N, Q, k


@pytest.mark.parametrize("dim,N,Q,k", list(_combos()))
def test_i8_search_grid(model, dim, N, Q, k):
    rng = np.random.default_rng(dim * 1000003 + N * 7 + Q * 3 + k)
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype="i8")
    if N:
        assert ix.add(rows) == 0
    assert len(ix) == N
    ids, sc = ix.search(queries, k)
    assert_exact(ids, sc, rows, queries, k)
    ix.close()


# ---- 2. ties and edge rows

def test_i8_ties_edge_rows_and_errors(model):
    rng = np.random.default_rng(5)
    dim = 96
    rows = unit_rows(rng, 400, dim)
    x = rows[17].copy()
    for i in (5, 17, 300, 301):
        rows[i] = x                                   # duplicates
    rows[50] = 2 * x                                  # the same codes at twice the scale
    rows[[60, 61]] = 0                                # all-zero rows
    rows[70] = x * np.float32(2.0 ** -60)
    rows[71] = x * np.float32(2.0 ** 60)
    rows[303] = np.nan
    rows[340, 7] = np.inf                             # one inf element: NaN scale, never returned
    rows[380, 0] = np.nan
    ix = model.index(dim=dim, dtype="i8")
    ix.add(rows)
    never = [303, 340, 380]
    ids, sc = ix.search(x[None], 10)
    assert ids[0, :6].tolist() == [71, 50, 5, 17, 300, 301]
    assert len(set(sc[0, 2:6].view(np.int32).tolist())) == 1            # identical bits for the duplicates
    assert_exact(ids, sc, rows, x[None], 10)
    q = np.concatenate([x[None], unit_rows(rng, 50, dim), np.zeros((1, dim), np.float32),
                        np.full((1, dim), np.nan, np.float32), np.zeros((1, dim), np.float32)])
    q[-1, 3] = np.inf
    for k in (1, 10, 256):
        ids, sc = ix.search(q, k)
        assert not np.isin(ids, never).any()
        assert_exact(ids, sc, rows, q, k)
    # a zero query: ids 0 .. k-1 at score 0; a NaN or inf query: nothing
    ids, sc = ix.search(q[-3:], 10)
    assert ids[0].tolist() == list(range(10)) and (sc[0] == 0).all()
    assert (ids[1:] == -1).all() and np.isneginf(sc[1:]).all()
    # fewer finite rows than k: those, then -1 / -inf
    small = model.index(dim=dim, dtype="i8")
    small.add(rows[300:310])
    ids, sc = small.search(q[:5], 20)
    assert ((ids >= 0).sum(axis=1) == 9).all()
    assert_exact(ids, sc, rows[300:310], q[:5], 20)
    # an empty index; k outside 1 .. 256
    empty = model.index(dim=dim, dtype="i8")
    ids, sc = empty.search(q[:2], 3)
    assert (ids == -1).all() and np.isneginf(sc).all()
    for bad in (0, 257):
        with pytest.raises(RuntimeError):
            ix.search(x[None], bad)
    for i in (ix, small, empty):
        i.close()


# ---- 3. invariance

def test_i8_bitwise_invariance(model):
    rng = np.random.default_rng(9)
    N, dim = 70001, 200
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, 1000, dim)
    ix = model.index(dim=dim, dtype="i8")
    ix.add(rows)
    ids, sc = ix.search(queries, 100)
    assert_exact(ids, sc, rows, queries, 100)
    for i in (0, 1, 577, 999):
        a_ids, a_sc = ix.search(queries[i:i + 1], 100)
        assert np.array_equal(a_ids[0], ids[i]) and np.array_equal(a_sc[0].view(np.int32), sc[i].view(np.int32))
    i10, s10 = ix.search(queries, 10)
    assert np.array_equal(i10, ids[:, :10]) and np.array_equal(s10.view(np.int32), sc[:, :10].view(np.int32))
    cuts = np.sort(rng.choice(np.arange(1, N), 36, replace=False))
    parts = model.index(dim=dim, dtype="i8")
    parts.reserve(N, 1000, 100)
    for p in np.split(rows, cuts):
        parts.add(p)
    assert len(parts) == N
    p_ids, p_sc = parts.search(queries, 100)
    assert np.array_equal(p_ids, ids) and np.array_equal(p_sc.view(np.int32), sc.view(np.int32))
    hip = _Hip()
    s = hip.stream()
    d_q, d_i, d_s = hip.upload(queries), hip.malloc(1000 * 100 * 4), hip.malloc(1000 * 100 * 4)
    ix.search_device(1000, d_q, 100, d_i, d_s, s)
    assert np.array_equal(hip.download(d_i, (1000, 100), np.int32), ids)
    assert np.array_equal(hip.download(d_s, (1000, 100)).view(np.int32), sc.view(np.int32))
    d_r = hip.upload(rows)
    dev = model.index(dim=dim, dtype="i8")
    assert dev.add_device(N, d_r, s) == 0
    dev.search_device(1000, d_q, 100, d_i, d_s, s)
    assert np.array_equal(hip.download(d_i, (1000, 100), np.int32), ids)
    assert np.array_equal(hip.download(d_s, (1000, 100)).view(np.int32), sc.view(np.int32))
    hip.free(d_q, d_i, d_s, d_r)
    for i in (ix, parts, dev):
        i.close()


# ---- 4. recall

def test_i8_recall_at_10(model):
    rng = np.random.default_rng(21)
    N, dim, Q, k = 200_000, 384, 200, 10
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype="i8")
    ix.add(rows)
    ids, sc = ix.search(queries, k)
    assert_exact(ids, sc, rows, queries, k)
    exact = queries.astype(np.float64) @ rows.astype(np.float64).T
    top = np.argsort(-exact, axis=1)[:, :k]
    recall = np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(ids, top)])
    assert recall >= 0.95, recall
    ix.close()


# ---- 5. text routes

def _texts():
    with open(TEXTS, encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f]


def test_i8_text_routes(make_model):
    path, _ = make_model("minilm-l6", "f16", 0)
    m = pybert.BertModel(path)
    texts = _texts()
    emb = m.encode_batch(texts)
    a = m.index(dtype="i8")
    assert a.add_texts(texts) == 0
    b = m.index(dtype="i8")
    b.add(emb)
    ia, sa = a.search(emb, 20)
    ib, sb = b.search(emb, 20)
    assert np.array_equal(ia, ib) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
    assert_exact(ia, sa, emb, emb, 20)
    queries = ["Should I get health insurance?", "poaching", texts[7], texts[123]]
    it, st = a.search_texts(queries, 5)
    ie, se = a.search(m.encode_batch(queries), 5)
    assert np.array_equal(it, ie) and np.array_equal(st.view(np.int32), se.view(np.int32))
    m.close()


# ---- 6. memory

def test_i8_memory_per_row(model):
    hip = _Hip()

    def taken(dtype):
        ix = model.index(dim=384, dtype=dtype)
        before = hip.free_bytes()
        ix.reserve(2_000_000, 1, 1)
        used = before - hip.free_bytes()
        ix.close()
        return used

    f16, i8 = taken("f16"), taken("i8")
    assert f16 >= 2_000_000 * 384 * 2, f16
    assert i8 <= 0.55 * f16, (i8, f16, i8 / f16)


# ---- 7. profile report

def test_i8_profile_names(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    rng = np.random.default_rng(2)
    ix = m.index(dim=64, dtype="i8")
    ix.add(unit_rows(rng, 5000, 64))
    ix.search(unit_rows(rng, 3, 64), 10)
    rep = m.profile_report()
    assert "index_quantize_i8" in rep and "index_topk_i8" in rep, sorted(rep)
    assert rep["index_topk_i8"]["launches"] >= 1
    m.close()


# ---- 8. the example

def test_i8_search_example_end_to_end(make_model):
    path, _ = make_model("minilm-l6", "f16", 0)
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    queries = ["Should I get health insurance?", "poaching"]
    r = subprocess.run([exe, "-m", path, "-f", TEXTS, "--i8"], input="\n".join(queries) + "\nq\n", capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loaded 600 lines." in r.stdout
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert len(blocks) == 2
    texts = _texts()
    m = pybert.BertModel(path)
    ix = m.index(dtype="i8")
    ix.add_texts(texts)
    want_i, want_s = ix.search_texts(queries, 3)
    for b, wi, ws in zip(blocks, want_i, want_s):
        lines = b.split("\n")
        got_t, got_s = [], []
        for j in range(3):
            assert lines[2 * j].startswith(f"{j + 1}. "), lines
            got_t.append(lines[2 * j][len(f"{j + 1}. "):])
            got_s.append(lines[2 * j + 1][len(" (similarity score: "):-1])
        assert got_s == [f"{x:.4f}" for x in ws]
        assert got_t == [texts[i] for i in wi]
    m.close()
