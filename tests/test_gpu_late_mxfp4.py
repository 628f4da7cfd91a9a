"""The token index's MXFP4 form (bert_hip_late_index_create dtype 4, "mxfp4": token_index.hip's token_mx_quantize_kernel and Mxfp4Form
on v_mfma_scale_f32_32x32x64_f8f6f4) against float64 NumPy over tests/mxfp4_reference.py: R[q][d] = sum_i max_j <Qd_i, Dd_j>.
The largest |score - R| / sum_i max_j (|Qd_i| . |Dd_j|) over the grid of test 3, measured on an MI355X: 1.12e-6 (dim 1024;
profiles/late_mxfp4_rate.txt).  That is below the 4.45e-5 measured for this instruction's chain in profiles/search_mxfp4_rate.txt, so
TOL stays the project's 8.9e-5, twice that figure."""
import numpy as np
import pytest

from bert_cpp_amd import pybert
from hip_graph import Hip
from mxfp4_reference import mxfp4_rows, mxfp8_queries
from test_gpu_search_b1 import assert_same, ref_topk, unit_rows
from test_gpu_search_mxfp4 import E2M1_TIES, _Hip, special

pytestmark = pytest.mark.gpu
TOL = 8.9e-5
DIMS = [8, 72, 128, 200, 384, 1024]
DOC_LENS, QUERY_LENS = [1, 31, 32, 33, 64, 65], [1, 32, 33, 128]


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.set_option("token_index_slices", "0")
    m.close()


def cu_of(lens, n):
    return np.concatenate([[0], np.cumsum(np.resize(lens, n))]).astype(np.int32)


def maxsim64(q, qcu, d, dcu):
    """float64 [n_q, n_docs] over the decoded operands: R = sum_i max_j <Qd_i, Dd_j>, and the two sums of the bound,
    sum_i max_j (|Qd_i| . |Dd_j|) and sum_i |max_j <Qd_i, Dd_j>|"""
    Q, D = mxfp8_queries(q).astype(np.float64), mxfp4_rows(d).astype(np.float64)
    M, A = np.maximum.reduceat(Q @ D.T, dcu[:-1], axis=1), np.maximum.reduceat(np.abs(Q) @ np.abs(D).T, dcu[:-1], axis=1)
    return tuple(np.add.reduceat(x, qcu[:-1], axis=0) for x in (M, A, np.abs(M)))


def index_of(model, d, dcu):
    ix = model.token_index(d.shape[1], "mxfp4")
    assert ix.add(d, dcu) == 0 and len(ix) == len(dcu) - 1 and model.lib.bert_hip_late_index_dtype(ix.ix) == 4
    return ix


@pytest.mark.parametrize("dim", DIMS)
def test_stored_form_bit_for_bit(model, dim):
    hip = Hip()
    x, cu = special(dim, E2M1_TIES, 8), np.array([0, 1, 3, 16], np.int32)
    x16 = (special(dim, E2M1_TIES, 6) * np.float32(2.0 ** -10)).astype(np.float16)     # (the six kinds that fit f16's range, 7.9 x 2^9 at the most)
    ix, dev = index_of(model, x, cu), model.token_index(dim, "mxfp4")
    d_rows = hip.upload(x16)
    assert dev.add_device(cu, d_rows) == 0
    hip.sync()
    for i in range(3):
        assert np.array_equal(ix.get_doc(i).view(np.int32), mxfp4_rows(x)[cu[i]:cu[i + 1]].view(np.int32)), i
        assert np.array_equal(dev.get_doc(i).view(np.int32), mxfp4_rows(x16.astype(np.float32))[cu[i]:cu[i + 1]].view(np.int32)), i
    hip.free(d_rows)
    ix.close(); dev.close()


@pytest.mark.parametrize("dim,N", [(8, 4500), (72, 63), (128, 64), (200, 4500), (384, 65), (1024, 1), (1024, 65)])
def test_exact_fit_ids_and_bits(model, dim, N):
    def ints(r, salt):                                               # the dense test's: integers in [-4, 4], every block's amax one of 1 .. 4
        i, r = np.arange(dim)[None, :], np.asarray(r)[:, None]
        cap = ((i // 32 + r) % 4 + 1).astype(np.float32)
        v = np.clip(((i * 7 + r * salt) % 9 - 4).astype(np.float32), -cap, cap)
        v[:, ::32] = cap[:, ::32]                                    # (the block's first element carries its amax)
        return v
    dcu, qcu = cu_of(DOC_LENS, N), cu_of(QUERY_LENS, 4)
    # a token's label: its place in the document and the document's id mod 5 — documents 30 apart are equal, so ties abound
    label = np.concatenate([np.arange(n) + 3 * (i % 5) for i, n in enumerate(np.diff(dcu))])
    rows = ints(label, 1) * np.float32(2.0) ** ((np.arange(dim)[None, :] // 32 * 5 + label[:, None]) % 7 - 3)
    q = ints(np.arange(qcu[-1]), 5)
    assert np.array_equal(mxfp4_rows(rows), rows) and np.array_equal(mxfp8_queries(q), q)
    R, A, _ = maxsim64(q, qcu, rows, dcu)                            # multiples of 2^-3 whose running sums stay below 2^24 of them
    assert (A * 8 < 2 ** 24).all()
    S = R.astype(np.float32)
    ix = index_of(model, rows, dcu)
    for k in (1, 10, 256):
        got = ix.search(q, qcu, k)
        assert_same(got, ref_topk(S, k), ("plain", k))
        assert_same(ix.rescore(q, qcu, got[0][:, ::-1], k), got, ("rescore", k))
    keep, allow = np.arange(N) % 3 != 0, np.arange(N) % 5 != 1
    keep[N // 8 // 32 * 32:N // 8 // 32 * 32 + 64] = False           # whole words without a qualifying document
    ix.remove(np.nonzero(~keep)[0])
    for k in (1, 10, 256):
        assert_same(ix.search(q, qcu, k, allow=allow), ref_topk(np.where(keep & allow, S, np.nan), k), ("removed and allowed", k))
    ix.close()


_WORST = [0.0]


@pytest.mark.parametrize("dim,N,k", [(8, 65, 10), (72, 64, 256), (128, 4500, 10), (200, 63, 1), (384, 300, 256), (1024, 65, 10)])
def test_random_unit_rows(model, dim, N, k):
    """the largest |score - R| / sum_i max_j (|Qd_i| . |Dd_j|) so far is printed by every case; over the grid, on an MI355X: 1.12e-6"""
    rng = np.random.default_rng(dim * 1000003 + N * 7 + k)
    dcu, qcu = cu_of(DOC_LENS, N), cu_of(QUERY_LENS, 4)
    d, q = unit_rows(rng, dcu[-1], dim), unit_rows(rng, qcu[-1], dim)
    ix = index_of(model, d, dcu)
    ids, sc = ix.search(q, qcu, k)
    ix.close()
    R, A, B = maxsim64(q, qcu, d, dcu)
    tol = TOL * A + np.diff(qcu)[:, None] * 2.0 ** -23 * B
    n = min(k, N)
    assert (ids[:, n:] == -1).all() and np.isneginf(sc[:, n:]).all() and (np.diff(sc[:, :n], axis=1) <= 0).all()
    for i in range(len(qcu) - 1):
        got = ids[i, :n]
        assert len(set(got.tolist())) == n and ((got >= 0) & (got < N)).all(), (i, got)
        _WORST[0] = max(_WORST[0], float((np.abs(sc[i, :n] - R[i, got]) / A[i, got]).max()))
        assert (np.abs(sc[i, :n] - R[i, got]) <= tol[i, got]).all(), (i, got, sc[i, :n], R[i, got])
        kth = np.sort(R[i])[::-1][n - 1]
        assert set(np.nonzero(R[i] > kth + 2 * tol[i])[0].tolist()) <= set(got.tolist()), i       # a clearly better document is returned
        assert (R[i, got] >= kth - 2 * tol[i, got]).all(), i                                        # and no clearly worse one
    print(f"largest |score - R| / sum_i max_j(|Qd_i| . |Dd_j|) so far: {_WORST[0]:.3e}")


def test_one_set_of_bits(model):
    rng, hip = np.random.default_rng(9), Hip()
    N, dim, Q = 4500, 200, 100
    dcu, qcu = cu_of(DOC_LENS, N), cu_of(QUERY_LENS, Q)
    d, q = unit_rows(rng, dcu[-1], dim).astype(np.float16).astype(np.float32), unit_rows(rng, qcu[-1], dim).astype(np.float16).astype(np.float32)
    ix = index_of(model, d, dcu)
    want = ix.search(q, qcu, 100)
    for i in (0, 57, 99):
        assert_same(ix.search(q[qcu[i]:qcu[i + 1]], [0, qcu[i + 1] - qcu[i]], 100), (want[0][i:i + 1], want[1][i:i + 1]), i)
    assert_same(ix.search(q, qcu, 10), (want[0][:, :10], want[1][:, :10]), "top-10 is a prefix of top-100")
    parts = model.token_index(dim, "mxfp4")
    for a, b in zip([0, 1, 700, 701, 3000], [1, 700, 701, 3000, N]):
        assert parts.add(d[dcu[a]:dcu[b]], dcu[a:b + 1] - dcu[a]) == a
    assert_same(parts.search(q, qcu, 100), want, "five adds")
    dev = model.token_index(dim, "mxfp4")
    d_rows, d_q, d_qcu = hip.upload(d.astype(np.float16)), hip.upload(q.astype(np.float16)), hip.upload(qcu)
    d_i, d_s = hip.nans((Q, 100), np.int32), hip.nans((Q, 100), np.float32)
    assert dev.add_device(dcu, d_rows) == 0
    dev.search_device(Q, d_qcu, d_q, 128, 100, d_i, d_s)
    assert_same((hip.download(d_i, (Q, 100), np.int32), hip.download(d_s, (Q, 100), np.float32)), want, "add_device, search_device")
    hip.free(d_rows, d_q, d_qcu, d_i, d_s)
    assert_same(ix.search(q, qcu, 100, allow=np.ones(N, bool)), want, "everything allowed")
    assert_same(ix.rescore(q, qcu, want[0], 100), want, "rescore")
    for slices in ("1", "7"):
        model.set_option("token_index_slices", slices)
        assert_same(ix.search(q, qcu, 100), want, ("token_index_slices", slices))
    model.set_option("token_index_slices", "0")
    for i in (ix, parts, dev):
        i.close()


def test_non_finite_input(model):
    rng = np.random.default_rng(5)
    dim, N = 104, 200
    dcu, qcu = cu_of([65, 1, 33], N), cu_of([33, 1, 40], 5)
    d, q = unit_rows(rng, dcu[-1], dim), unit_rows(rng, qcu[-1], dim)
    bad = [3, 42, 84, 123, 199]                                      # of 65, 65, 65, 65 and 1 tokens
    # the first token (first block), a middle one (second block), the last (last block), the last of the first block, a lone token
    for doc, t, e, v in zip(bad, [0, 40, 64, 31, 0], [0, 50, 103, 70, 33], [np.nan, np.inf, -np.inf, np.nan, np.inf]):
        d[dcu[doc] + t, e] = v
    q[qcu[1], 103], q[qcu[3] + 32, 0] = np.nan, np.inf            # a lone token; the last of 33, in the second block
    ix = index_of(model, d, dcu)
    assert all(np.isnan(ix.get_doc(b)).any() for b in bad)
    ids, sc = ix.search(q, qcu, 256)                                 # k >= N: every document that can be returned is
    assert (ids[[1, 3]] == -1).all() and np.isneginf(sc[[1, 3]]).all()
    for i in (0, 2, 4):
        assert set(ids[i, :N - 5].tolist()) == set(range(N)) - set(bad) and (ids[i, N - 5:] == -1).all()
        assert_same(ix.search(q[qcu[i]:qcu[i + 1]], [0, qcu[i + 1] - qcu[i]], 256), (ids[i:i + 1], sc[i:i + 1]), "beside a NaN query")
    ix.close()


def test_edges_of_the_surface(make_model, tmp_path, capfd):
    m = pybert.BertModel(make_model("tiny", "f16", 0)[0])
    m.profile(True)
    hip, dev, rng = _Hip(), Hip(), np.random.default_rng(2)
    big = m.token_index(384, "mxfp4")
    used = hip.free_bytes()
    big.reserve(1, 2_000_000)
    used -= hip.free_bytes()
    big.close()
    assert 2_000_000 * 208 - 2 * (2 << 20) < used <= 2_000_000 * 208 + (16 << 20), used       # (free memory counted in 2 MiB pages)
    dcu = cu_of(DOC_LENS, 100)
    for dim in (128, 1024):
        ix = index_of(m, unit_rows(rng, dcu[-1], dim), dcu)
        assert ix.max_query_tokens() == 128
        with pytest.raises(ValueError):                              # a longer query: refused by the host form,
            ix.search(unit_rows(rng, 129, dim), [0, 129], 4)
        # the guards' lists from the device form's rescore, which sizes its launch for max_query_tokens
        d_q, d_qcu = dev.upload(unit_rows(rng, 134, dim).astype(np.float16)), dev.upload(np.array([0, 129, 134], np.int32))
        d_c = dev.upload(np.tile(np.arange(100, dtype=np.int32), (2, 1)))
        d_i, d_s = dev.nans((2, 4), np.int32), dev.nans((2, 4), np.float32)
        ix.rescore_device(2, d_qcu, d_q, 100, d_c, 4, d_i, d_s)
        ids, sc = dev.download(d_i, (2, 4), np.int32), dev.download(d_s, (2, 4), np.float32)
        assert (ids[0] == -1).all() and np.isneginf(sc[0]).all() and (ids[1] >= 0).all()
        dev.free(d_q, d_qcu, d_c, d_i, d_s)
    q, qcu = unit_rows(rng, 40, 1024), [0, 7, 40]
    before = ix.search(q, qcu, 10)
    capfd.readouterr()
    for call, line in ((lambda: ix.get_codes(0), "mxfp4 rows"), (ix.compact, "compact: not available for an mxfp4 token index"),
                       (lambda: ix.save(str(tmp_path / "no.tok")), "save: not available for an mxfp4 token index")):
        with pytest.raises(ValueError):
            call()
        assert line in capfd.readouterr().err
    # a refusal writes no file and leaves the index as it was
    assert not list(tmp_path.iterdir())
    got = ix.search(q, qcu, 10)
    assert_same(got, before, "after the refusals")
    assert ix.remove([1]) == 1 and ix.search(q, qcu, 10) and ix.rescore(q, qcu, got[0], 5)
    rep = m.profile_report()
    for name in ("token_mx_quantize", "token_mxfp4_scan", "token_mxfp4_scan_masked", "token_mxfp4_rescore"):
        assert name in rep and rep[name]["launches"] >= 1, (name, sorted(rep))
    ix.close()
    m.close()
