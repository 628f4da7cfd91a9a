"""Embedding index and its top-k search on the GPU (bert_hip_index_*, search.hip) against NumPy float64 on the stored values
(f16-rounded rows and queries for the f16 index).  Per score the tolerance is tol = 2e-6 * sum_i |q_i r_i|: a figure for
Gaussian data, not a bound of the arithmetic — over 2048 products of one sign (a query that is a row's own direction at dim
2048) a correctly rounded f32 fma chain in the kernel's order reaches 1.07 of it (tests/index_reference.py, f32_chain_scores).  The exact
scores are float64 over the rows a float32 screen keeps (every row within 1e-3 of the screened k-th score), so that the
million-row cases stay small on the host."""
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


def stored(x, dtype):
    return x.astype(np.float16).astype(np.float32) if dtype == "f16" else np.asarray(x, dtype=np.float32)


def check_results(ids, scores, rows, queries, k, dtype):
    R, Q = stored(rows, dtype), stored(queries, dtype)
    N = R.shape[0]
    valid_rows = ~np.isnan(R).any(axis=1) if N else np.zeros(0, bool)
    n_ret = min(k, int(valid_rows.sum()))
    assert ids.shape == (Q.shape[0], k) and scores.shape == (Q.shape[0], k)
    for b0 in range(0, Q.shape[0], 16):
        qb = Q[b0:b0 + 16]
        s32 = qb @ R.T if N else np.zeros((len(qb), 0), np.float32)
        for j, q in enumerate(qb):
            i, row_ids, row_sc = b0 + j, ids[b0 + j], scores[b0 + j]
            # the tail: -1 / -inf
            assert (row_ids[n_ret:] == -1).all() and np.isneginf(row_sc[n_ret:]).all(), (i, row_ids, row_sc)
            got = row_ids[:n_ret]
            assert len(set(got.tolist())) == n_ret and ((got >= 0) & (got < N)).all(), (i, got)
            assert (np.diff(row_sc[:n_ret]) <= 0).all(), (i, row_sc)
            if n_ret == 0:
                continue
            sc = np.where(valid_rows, s32[j], -np.inf)
            kth32 = np.partition(sc, N - n_ret)[N - n_ret]
            cand = np.union1d(np.nonzero(sc >= kth32 - 1e-3)[0], got)
            q64, r64 = q.astype(np.float64), R[cand].astype(np.float64)
            exact, tol = r64 @ q64, 2e-6 * (np.abs(r64) @ np.abs(q64))
            ex = dict(zip(cand.tolist(), exact)); tl = dict(zip(cand.tolist(), tol))
            for g, s in zip(got.tolist(), row_sc[:n_ret]):
                assert abs(float(s) - ex[g]) <= tl[g] + 1e-30, (i, g, float(s), ex[g])
            kth = np.sort(exact)[::-1][n_ret - 1]
            gs = set(got.tolist())
            for c, e, t in zip(cand.tolist(), exact, tol):
                if e > kth + 2 * t:
                    assert c in gs, (i, c, e, kth)
            for g in got.tolist():
                assert ex[g] >= kth - 2 * tl[g], (i, g, ex[g], kth)


def _combos():
    dims = [1, 7, 64, 130, 384, 768, 1024, 2048]
    per_dim = {                     # (N, Q, k), pruned so that every value of each axis appears with small and large dims
        1: [(0, 3, 10), (31, 64, 256), (1000, 1, 1)],
        7: [(1, 1, 10), (1000, 1000, 100), (65537, 3, 256)],
        64: [(31, 3, 1), (65537, 64, 10), (1000, 1000, 256)],
        130: [(0, 1, 1), (1000, 64, 100), (65537, 1, 10)],
        384: [(1, 64, 256), (31, 1000, 10), (65537, 1000, 100)],
        768: [(1000, 3, 10), (65537, 64, 1), (31, 1, 100)],
        1024: [(0, 64, 256), (1000, 1, 100), (65537, 3, 10)],
        2048: [(31, 3, 256), (1000, 64, 10), (65537, 1, 100)],
    }
    for dtype in ("f32", "f16"):
        for d in dims:
            for N, Q, k in per_dim[d]:
                yield dtype, d, N, Q, k


@pytest.mark.parametrize("dtype,dim,N,Q,k", list(_combos()))
def test_search_grid(model, dtype, dim, N, Q, k):
    rng = np.random.default_rng(dim * 1000003 + N * 7 + Q * 3 + k)
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype=dtype)
    if N:
        assert ix.add(rows) == 0
    assert len(ix) == N
    ids, scores = ix.search(queries, k)
    check_results(ids, scores, rows, queries, k, dtype)
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_search_full_size(model, dtype):
    rng = np.random.default_rng(11)
    N, dim, Q, k = 1_000_003, 384, 257, 100
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    ids, scores = ix.search(queries, k)
    check_results(ids, scores, rows, queries, k, dtype)
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ties_by_id_and_nan_rows_never_returned(model, dtype):
    rng = np.random.default_rng(5)
    dim = 96
    rows = unit_rows(rng, 400, dim)
    x = rows[17].copy()
    for i in (5, 17, 300, 301):
        rows[i] = x
    rows[[3, 40, 200]] = np.nan
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    for k in (2, 4, 10):
        ids, sc = ix.search(x[None], k)
        want = [5, 17, 300, 301][:k]
        assert ids[0, :len(want)].tolist() == want
        assert len(set(sc[0, :len(want)].view(np.int32).tolist())) == 1          # identical bits
    q50 = unit_rows(rng, 50, dim)
    ids, sc = ix.search(q50, 256)
    assert not np.isin(ids, [3, 40, 200]).any()
    check_results(ids, sc, rows, q50, 256, dtype)
    # k beyond the rows that have a score (29 of 30): those, then -1 / -inf
    small = model.index(dim=dim, dtype=dtype)
    small.add(rows[:30])
    ids, sc = small.search(q50, 100)
    assert ((ids >= 0).sum(axis=1) == 29).all() and not np.isin(ids, [3]).any()
    check_results(ids, sc, rows[:30], q50, 100, dtype)
    small.close()
    # an index of NaN rows only: nothing to return
    nan_ix = model.index(dim=dim, dtype=dtype)
    nan_ix.add(np.full((70, dim), np.nan, np.float32))
    ids, sc = nan_ix.search(unit_rows(rng, 3, dim), 5)
    assert (ids == -1).all() and np.isneginf(sc).all()
    # an empty index is valid; k outside 1 .. 256 is an error; no queries is a no-op
    empty = model.index(dim=dim, dtype=dtype)
    ids, sc = empty.search(unit_rows(rng, 2, dim), 3)
    assert (ids == -1).all() and np.isneginf(sc).all()
    for bad in (0, 257):
        with pytest.raises(RuntimeError):
            ix.search(x[None], bad)
    ids, sc = ix.search(np.zeros((0, dim), np.float32), 4)
    assert ids.shape == (0, 4)
    for i in (ix, nan_ix, empty):
        i.close()


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


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_bitwise_invariance(model, dtype):
    rng = np.random.default_rng(9)
    N, dim = 70001, 200
    rows, queries = unit_rows(rng, N, dim), unit_rows(rng, 1000, dim)
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    ids, sc = ix.search(queries, 100)
    # a query alone or inside the batch of 1000
    for i in (0, 1, 577, 999):
        a_ids, a_sc = ix.search(queries[i:i + 1], 100)
        assert np.array_equal(a_ids[0], ids[i]) and np.array_equal(a_sc[0].view(np.int32), sc[i].view(np.int32))
    # k = 10 is the first 10 of k = 100
    i10, s10 = ix.search(queries, 10)
    assert np.array_equal(i10, ids[:, :10]) and np.array_equal(s10.view(np.int32), sc[:, :10].view(np.int32))
    # 37 add calls of uneven size, and storage reserved up front, against one add into grown storage
    cuts = np.sort(rng.choice(np.arange(1, N), 36, replace=False))
    parts = model.index(dim=dim, dtype=dtype)
    parts.reserve(N, 1000, 100)
    for p in np.split(rows, cuts):
        parts.add(p)
    assert len(parts) == N
    p_ids, p_sc = parts.search(queries, 100)
    assert np.array_equal(p_ids, ids) and np.array_equal(p_sc.view(np.int32), sc.view(np.int32))
    # search_device on a stream of the caller's own: the same bits
    hip = _Hip()
    s = hip.stream()
    d_q, d_i, d_s = hip.upload(queries), hip.malloc(1000 * 100 * 4), hip.malloc(1000 * 100 * 4)
    ix.search_device(1000, d_q, 100, d_i, d_s, s)
    assert np.array_equal(hip.download(d_i, (1000, 100), np.int32), ids)
    assert np.array_equal(hip.download(d_s, (1000, 100)).view(np.int32), sc.view(np.int32))
    # add_device from device rows: the same index
    d_r = hip.upload(rows)
    dev = model.index(dim=dim, dtype=dtype)
    assert dev.add_device(N, d_r, s) == 0
    dev.search_device(1000, d_q, 100, d_i, d_s, s)
    assert np.array_equal(hip.download(d_i, (1000, 100), np.int32), ids)
    assert np.array_equal(hip.download(d_s, (1000, 100)).view(np.int32), sc.view(np.int32))
    hip.free(d_q, d_i, d_s, d_r)
    for i in (ix, parts, dev):
        i.close()


def test_forward_pass_then_search_on_one_stream_without_a_host_sync(make_model):
    """bert_hip_eval_packed_device -> bert_hip_index_search_device enqueued back to back on one stream, nothing in between:
    the results are those of the host route on the same embeddings."""
    path, hp = make_model("minilm-l6", "f16", 0)
    m = pybert.BertModel(path)
    hip = _Hip()
    rng = np.random.default_rng(3)
    lens = rng.integers(5, 60, 300)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T, B, H = int(cu[-1]), len(lens), hp.n_embd
    toks = rng.integers(1000, hp.n_vocab, size=T).astype(np.int32)
    emb = m.eval_packed(toks, cu)
    ix = m.index(dtype="f32")
    ix.add(emb)
    want_i, want_s = ix.search(emb, 10)
    s = hip.stream()
    d_t, d_cu, d_e = hip.upload(toks), hip.upload(cu), hip.malloc(B * H * 4)
    d_i, d_s = hip.malloc(B * 10 * 4), hip.malloc(B * 10 * 4)
    m.reserve(T, B)
    ix.reserve(B, B, 10)
    m.eval_packed_device(d_t, d_cu, B, T, 128, d_e, s)
    ix.search_device(B, d_e, 10, d_i, d_s, s)
    assert np.array_equal(hip.download(d_i, (B, 10), np.int32), want_i)
    assert np.array_equal(hip.download(d_s, (B, 10)).view(np.int32), want_s.view(np.int32))
    hip.free(d_t, d_cu, d_e, d_i, d_s)
    m.close()                      # (frees the index)


def _texts():
    with open(TEXTS, encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f]


def test_text_routes_with_the_engine(make_model):
    path, _ = make_model("minilm-l6", "f16", 0)
    m = pybert.BertModel(path)
    texts = _texts()
    emb = m.encode_batch(texts)
    a = m.index(dtype="f32")
    assert a.add_texts(texts) == 0
    b = m.index(dtype="f32")
    b.add(emb)
    # the stored rows are the same bits: every search agrees to the bit
    ia, sa = a.search(emb, 20)
    ib, sb = b.search(emb, 20)
    assert np.array_equal(ia, ib) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
    queries = ["Should I get health insurance?", "poaching", texts[7], texts[123]]
    it, st = a.search_texts(queries, 5)
    ie, se = a.search(m.encode_batch(queries), 5)
    assert np.array_equal(it, ie) and np.array_equal(st.view(np.int32), se.view(np.int32))
    # each text finds itself: the smallest id with the same embedding, at its own score
    i1, s1 = a.search_texts(texts, 1)
    for i in range(len(texts)):
        same = [j for j in range(len(texts)) if np.array_equal(emb[j], emb[i])]
        assert i1[i, 0] == same[0], (i, texts[i], texts[i1[i, 0]])
        assert texts.index(texts[i]) >= same[0]
        assert s1[i, 0] == sa[i][ia[i] == same[0]][0]
    m.close()


def test_search_example_end_to_end(make_model):
    path, _ = make_model("minilm-l6", "f16", 0)
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    queries = ["Should I get health insurance?", "poaching"]
    r = subprocess.run([exe, "-m", path, "-f", TEXTS], input="\n".join(queries) + "\nq\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Loaded 600 lines." in r.stdout
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert len(blocks) == 2
    texts = _texts()
    m = pybert.BertModel(path)
    ix = m.index()
    ix.add_texts(texts)
    want_i, want_s = ix.search_texts(queries, 3)
    for b, wi, ws in zip(blocks, want_i, want_s):
        lines = b.split("\n")
        got_t, got_s = [], []
        for j in range(3):
            assert lines[2 * j].startswith(f"{j + 1}. "), lines
            got_t.append(lines[2 * j][len(f"{j + 1}. "):])
            assert lines[2 * j + 1].startswith(" (similarity score: ") and lines[2 * j + 1].endswith(")")
            got_s.append(lines[2 * j + 1][len(" (similarity score: "):-1])
        assert [float(x) for x in got_s] == sorted((float(x) for x in got_s), reverse=True)
        assert got_s == [f"{x:.4f}" for x in ws]
        assert got_t == [texts[i] for i in wi]
    m.close()
