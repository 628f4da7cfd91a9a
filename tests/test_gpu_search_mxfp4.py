"""The MXFP4 embedding index (bert_hip_index_create dtype 4, "mxfp4": search.hip's index_quantize_mx_kernel and
ScoreBlock<mxfp4_t> on v_mfma_scale_f32_32x32x64_f8f6f4) against tests/mxfp4_reference.py.
Recall of the exact top-10 among this form's own best 10 / 20 / 50 candidates, unit Gaussian rows, 10^5 rows, dim 384, 200
queries, in NumPy with the reference: 0.78 / 0.965 / 1.00 (b1: 0.17 / 0.26 / 0.40; i8's own top-10: 0.98); nothing is gated on it.
The largest |score - exact| / sum_i |q_i r_i| over the grid of test 3, measured on an MI355X: 4.45e-5 (dim 33; mean 2e-7;
profiles/search_mxfp4_rate.txt), above the 2e-6 of an f32 chain of exact products: the scaled MFMA's sum over its 64 products
is narrower than f32.  TOL is twice the measured figure."""
import os

import numpy as np
import pytest

from bert_cpp_amd import pybert
from mxfp4_reference import mxfp4_rows, mxfp8_queries
from test_gpu_search_b1 import TEXTS, _Hip, assert_same, model, ref_topk, unit_rows  # noqa: F401 (model: the fixture)

pytestmark = pytest.mark.gpu
TOL = 8.9e-5
GRID = [(d, *c) for d, cs in {1: [(0, 1, 10), (127, 31, 256), (4500, 100, 1)], 31: [(1, 32, 1), (128, 33, 10), (4500, 1, 256)],
                              33: [(129, 100, 256), (1, 1, 10), (127, 32, 1)], 64: [(4500, 33, 10), (128, 1, 1), (129, 31, 256)],
                              65: [(127, 100, 10), (4500, 32, 256), (0, 33, 1)], 384: [(4500, 100, 10), (129, 1, 256), (128, 31, 1)],
                              2048: [(127, 33, 10), (4500, 1, 1), (129, 32, 256)]}.items() for c in cs]
E2M1_TIES = [2.5, -3.5, 5, 0.25, 4, -0.75, 1.25, 1.75]
# against an amax of 470 (e = 0): mantissa ties (17 -> 16, 19 -> 20, 2^-7 + 2^-11 -> 2^-7), subnormal ties (1.5, 2.5 -> 2 x 2^-9), 460, 470 -> 448
E4M3_TIES = [17, -19, 1.5 * 2.0 ** -9, -2.5 * 2.0 ** -9, 460, -470, 2.0 ** -7 + 2.0 ** -11, 448]


def index_of(model, rows, dim):
    ix = model.index(dim=dim, dtype="mxfp4")
    assert len(rows) == 0 or ix.add(rows) == 0
    return ix


def special(dim, ties, kinds):
    """[16, dim]: every kind of block in every block position — zero, amax a power of two, amax just below one (saturates), rounding
    ties, a 2^40 dynamic range, plain, and (kinds = 8) amax subnormal and amax near FLT_MAX"""
    rng, nb = np.random.default_rng(dim), (dim + 31) // 32
    x = np.zeros((16, nb * 32), np.float32)
    for r, b in np.ndindex(16, nb):
        u = rng.uniform(-1, 1, 32).astype(np.float32)
        s = np.float32(2.0) ** int(rng.integers(-20, 20))
        x[r, 32 * b:32 * b + 32] = [np.zeros(32), u / np.abs(u).max() * 4 * s, u / np.abs(u).max() * np.float32(7.9) * s, np.resize(np.float32(ties), 32) * s,
                                    u * np.float32(2.0) ** rng.integers(-40, 1, 32), u, u * np.float32(2.0 ** -140), u * np.float32(3e38)][(r + b) % kinds]
    return x[:, :dim]


@pytest.mark.parametrize("dim", [1, 31, 33, 64, 65, 384, 2048])
def test_stored_form_bit_for_bit(model, dim):
    x = special(dim, E2M1_TIES, 8)
    ix = index_of(model, x, dim)
    assert np.array_equal(ix.get_rows(np.arange(16)).view(np.int32), mxfp4_rows(x).view(np.int32))
    ix.close()


def test_query_form_bit_for_bit(model):
    # row r holds one power of two at element r: its score is that product alone, so a search with k = N reads the stored query back
    dim = 200
    x = special(dim, E4M3_TIES, 6)
    val = (np.float32(2.0) ** (np.arange(dim) % 5 - 4) * (-1) ** np.arange(dim)).astype(np.float32)
    ix = index_of(model, np.diag(val), dim)
    ids, sc = ix.search(x, dim)
    got = np.full((16, dim), np.nan, np.float32)
    np.put_along_axis(got, ids, sc, axis=1)
    assert (np.sort(ids, axis=1) == np.arange(dim)).all() and np.array_equal(got, mxfp8_queries(x) * val)
    ix.close()


@pytest.mark.parametrize("dim,N,Q", [(1, 127, 31), (31, 128, 33), (33, 129, 100), (64, 4500, 33), (65, 127, 1), (384, 4500, 100), (2048, 300, 32)])
def test_exact_fit_ids_and_bits(model, dim, N, Q):
    def ints(n, salt):                                               # integers in [-4, 4], every block's amax one of 1 .. 4
        i, r = np.arange(dim)[None, :], np.arange(n)[:, None]
        cap = ((i // 32 + r) % 4 + 1).astype(np.float32)
        v = np.clip(((i * 7 + r * salt) % 9 - 4).astype(np.float32), -cap, cap)
        v[:, ::32] = cap[:, ::32]                                    # (the block's first element carries its amax)
        return v
    rows = ints(N, 1) * np.float32(2.0) ** ((np.arange(dim)[None, :] // 32 * 5 + np.arange(N)[:, None]) % 7 - 3)
    q = ints(Q, 5)
    ix = index_of(model, rows, dim)
    assert np.array_equal(ix.get_rows(np.arange(N)), rows) and np.array_equal(mxfp8_queries(q), q) and np.array_equal(mxfp4_rows(rows), rows)
    S = (q.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)        # integers times 2^-3, below 2^24
    keep, allow = np.arange(N) % 3 != 0, np.arange(N) % 5 != 1
    keep[N // 8 // 32 * 32:N // 8 // 32 * 32 + 64] = False                             # whole words without a qualifying row
    for k in (1, 10, 256):
        assert_same(ix.search(q, k), ref_topk(S, k), ("plain", k))
    ix.remove(np.nonzero(~keep)[0])
    for k in (1, 10, 256):
        assert_same(ix.search(q, k, allow=allow), ref_topk(np.where(keep & allow, S, np.nan), k), ("removed and allowed", k))
    old = ix.compact()
    for k in (1, 10, 256):
        assert_same(ix.search(q, k), ref_topk(S[:, old], k), ("compacted", k))
    ix.close()


@pytest.mark.parametrize("dim,N,Q,k", GRID)
def test_random_unit_rows(model, dim, N, Q, k):
    rng = np.random.default_rng(dim * 1000003 + N * 7 + Q * 3 + k)
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ids, sc = index_of(model, rows, dim).search(q, k)
    # tests/test_gpu_search.py's three conditions against float64 over the decoded operands, every row a candidate
    R, Qd = mxfp4_rows(rows).astype(np.float64), mxfp8_queries(q).astype(np.float64)
    exact, tol = Qd @ R.T, TOL * (np.abs(Qd) @ np.abs(R).T) + 1e-30
    n = min(k, N)
    assert (ids[:, n:] == -1).all() and np.isneginf(sc[:, n:]).all() and (np.diff(sc[:, :n], axis=1) <= 0).all()
    for i in range(Q if n else 0):
        got = ids[i, :n]
        assert len(set(got.tolist())) == n and ((got >= 0) & (got < N)).all(), (i, got)
        assert (np.abs(sc[i, :n] - exact[i, got]) <= tol[i, got]).all(), (i, got, sc[i, :n], exact[i, got])
        kth = np.sort(exact[i])[::-1][n - 1]
        assert set(np.nonzero(exact[i] > kth + 2 * tol[i])[0].tolist()) <= set(got.tolist()), i     # a clearly better row is returned
        assert (exact[i, got] >= kth - 2 * tol[i, got]).all(), i                                      # and no clearly worse one


def test_one_set_of_bits(model):
    rng = np.random.default_rng(9)
    N, dim, Q = 4500, 200, 100
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    ix = index_of(model, rows, dim)
    want = ix.search(q, 100)
    for i in (0, 57, 99):
        assert_same(ix.search(q[i:i + 1], 100), (want[0][i:i + 1], want[1][i:i + 1]), i)
    assert_same(ix.search(q, 10), (want[0][:, :10], want[1][:, :10]), "top-10 is a prefix of top-100")
    parts = model.index(dim=dim, dtype="mxfp4")
    parts.reserve(N, Q, 100)
    for p in np.split(rows, [1, 700, 701, 3000]):
        parts.add(p)
    assert_same(parts.search(q, 100), want, "parts")
    hip = _Hip()
    s, d_q, d_i, d_s, d_r = hip.stream(), hip.upload(q), hip.malloc(Q * 100 * 4), hip.malloc(Q * 100 * 4), hip.upload(rows)
    dev = model.index(dim=dim, dtype="mxfp4")
    assert dev.add_device(N, d_r, s) == 0
    dev.search_device(Q, d_q, 100, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, 100), np.int32), hip.download(d_s, (Q, 100))), want, "add_device, search_device")
    hip.free(d_q, d_i, d_s, d_r)
    assert_same(ix.rescore(q, want[0][:, ::-1], 100), want, "rescore")
    fine = model.index(dim=dim, dtype="f16")
    assert fine.add(rows) == 0
    assert_same(ix.search_rescored(fine, q, 10, 50), fine.rescore(q, ix.search(q, 50)[0], 10), "search_rescored")
    ix.train_partition(8, 2)
    assert_same(ix.search_probed(q, 100, nprobe=8), want, "every list probed")
    sp = model.sparse_index(4, "f32", n_vocab=50)
    sp.add(rng.permuted(np.tile(np.arange(50), (N, 1)), axis=1)[:, :4], rng.random((N, 4), dtype=np.float32))
    assert_same(ix.hybrid_search(sp, q, np.tile(np.arange(4), (Q, 1)), np.ones((Q, 4), np.float32), 100, 1.0, 0.0), want, "hybrid (1, 0)")
    for i in (ix, parts, dev, fine, sp):
        i.close()


def test_non_finite_input(model):
    rng = np.random.default_rng(5)
    dim, N, bad = 100, 200, [3, 43, 83, 123]
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, 5, dim)
    rows[bad, [0, 50, 99, 70]] = [np.nan, np.inf, -np.inf, np.nan]                    # first, middle, padding-adjacent block
    q[1, 99], q[3, 0] = np.nan, np.inf
    ix = index_of(model, rows, dim)
    assert np.isnan(ix.get_rows(bad)).all()
    ids, sc = ix.search(q, 256)                                      # k >= N: every row that can be returned is
    assert (ids[[1, 3]] == -1).all() and np.isneginf(sc[[1, 3]]).all()
    for i in (0, 2, 4):
        assert set(ids[i, :N - 4].tolist()) == set(range(N)) - set(bad) and (ids[i, N - 4:] == -1).all()
        assert_same(ix.search(q[i:i + 1], 256), (ids[i:i + 1], sc[i:i + 1]), "beside a NaN query")
    ix.close()


def test_edges_of_the_surface(make_model, tmp_path, capfd):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    hip, rng = _Hip(), np.random.default_rng(2)
    big = m.index(dim=384, dtype="mxfp4")
    used = hip.free_bytes()
    big.reserve(2_000_000, 1, 1)
    used -= hip.free_bytes()
    big.close()
    assert 2_000_000 * 208 - 2 * (2 << 20) < used <= 2_000_000 * 208 + (16 << 20), used       # (b1's test: 2 MiB pages)
    ix = index_of(m, unit_rows(rng, 5000, 64), 64)
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        ix.save(str(tmp_path / "no.idx"))
    assert "no file form yet" in capfd.readouterr().err and not os.listdir(tmp_path)
    assert ix.search(unit_rows(rng, 3, 64), 10) and ix.remove([1]) == 1 and ix.search(unit_rows(rng, 3, 64), 10)
    rep = m.profile_report()
    for name in ("index_quantize_mxfp4", "index_quantize_mxfp8", "index_topk_mxfp4", "index_topk_mxfp4_masked"):
        assert name in rep and rep[name]["launches"] >= 1, (name, sorted(rep))
    texts = open(TEXTS, encoding="utf-8").read().splitlines()[:150]
    emb = m.encode_batch(texts)
    a, b = m.index(dtype="mxfp4"), m.index(dtype="mxfp4")
    assert a.add_texts(texts) == 0 and b.add(emb) == 0
    assert_same(a.search(emb, 20), b.search(emb, 20), "add_texts against encode + add")
    m.close()
