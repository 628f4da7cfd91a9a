"""The hybrid search's two kernels on ordered and exact-fit scores: sparse_hybrid_scan_kernel<DTYPE, MASKED> (sparse_index.hip), the
second pass, behind index_scores_kernel<T, MASKED> and mask_and_kernel (search.hip), through BertIndex.hybrid_search.  The fixtures are
tests/topk_order_reference.py's hybrid ones: scores that are an exact, known function of the row id, carried by both indexes together
(split), by the dense one alone or by the sparse one alone.  Every comparison is bit for bit in ids and scores against
hybrid_reference.search over D and S of the two stored forms' references — index_reference and sparse_index_reference, never a kernel
of this library.

Random scores fill the scan's queue once; these fill it at every step, fill it exactly (count == room: the step is not sorted and the
next one writes up to the list's last slot), miss that by one row, keep one query of a tile busy beside idle ones, tie over the whole
index, and are ordered by D and S together: neither term alone, nor the weights swapped, gives the top-k of H.
test_topk_order_host.py proves on the CPU, under the plan the search itself makes, that each fixture used here reaches its state."""
import numpy as np
import pytest

import index_reference as ixr
import topk_order_reference as tor

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    """any model: both indexes only need the context's device.  It profiles, so that the last test can show which kernels this file ran."""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    yield m
    m.close()


def pair(model, fx, gone_dense=(), gone_sparse=()):
    """the two indexes of a fixture, rows removed on either side"""
    dix = model.index(dim=fx.rows.shape[1], dtype=fx.dd)
    six = model.sparse_index(fx.width, fx.sd, n_vocab=tor.SPARSE_V)
    assert dix.add(fx.rows) == 0 and six.add(fx.term_ids, fx.term_w) == 0 and len(dix) == len(six) == fx.n
    if len(gone_dense):
        assert dix.remove(gone_dense) == len(gone_dense)
    if len(gone_sparse):
        assert six.remove(gone_sparse) == len(gone_sparse)
    return dix, six


def tile_of(fx, nq, k, pref=0):
    """the scan's tile under the plan of the call's first chunk"""
    chunks, _ = tor.hybrid_chunks(fx.n, nq, pref, pybert.test_hybrid_chunk)
    return pybert.test_sparse_scan_geometry(tor.SPARSE_DTYPES.index(fx.sd), tor.SPARSE_V, fx.n, chunks[0][1], k)["qb"]


def run_layouts(dix, six, fx, k, nqs, allow=None, qual=None, pref=0, what=""):
    """every layout of every nq against the reference over the rows qual (None: the fixture's); returns the results by (nq, layout)"""
    want = tor.hybrid_reference(fx, k, qual)
    out = {}
    for nq in nqs:
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tile_of(fx, nq, k, pref)).items():
            got = dix.hybrid_search(six, *tor.hybrid_queries(fx, lay), k, fx.w[0], fx.w[1], allow=allow)
            ixr.assert_same(got, tor.of_layout(want, lay), (fx.name, what, nq, name))
            out[(nq, name)] = got
    return out


# ------------------------------------------------------------------------------------------------
# the queue states of the four scan instantiations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", tor.HYBRID_KS)
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
def test_hybrid_search_on_ordered_and_exact_fit_rows(model, sd, k, mode):
    """the split carrier, dense f32 beside sparse f32 and f16 beside f16, under every weight pair"""
    for w in tor.HYBRID_WEIGHTS:
        fx = tor.hybrid_split_fixture(sd, sd, k, mode, w)
        if mode == "removed":
            # the rows that must not qualify: a third removed from the dense index, a third from the sparse one, a third disallowed
            gone_d, gone_s, allow = tor.hybrid_removed_split(fx.ok, True)
            dix, six = pair(model, fx, gone_d, gone_s)
            assert dix.n_live == fx.n - len(gone_d)
            run_layouts(dix, six, fx, k, tor.HYBRID_NQS, allow=allow, what="three bitmaps")
            dix.close()
            six.close()
            # all of them removed in the sparse index alone; then disallowed as well
            dix, six = pair(model, fx, gone_sparse=tor.hybrid_removed_split(fx.ok, False)[1])
            run_layouts(dix, six, fx, k, tor.HYBRID_NQS, what="removed in the sparse index")
            run_layouts(dix, six, fx, k, tor.HYBRID_NQS, allow=fx.ok, what="removed in the sparse index and disallowed")
        else:
            dix, six = pair(model, fx)
            run_layouts(dix, six, fx, k, tor.HYBRID_NQS, allow=fx.ok)
            if mode == "allow":                                      # the near miss on the same pair: one row more than fits
                run_layouts(dix, six, fx, k, tor.HYBRID_NQS, allow=fx.ok1, qual=fx.ok1, what="near miss")
        dix.close()
        six.close()


# ------------------------------------------------------------------------------------------------
# the dense pass in all its forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("k", tor.HYBRID_DENSE_KS)
@pytest.mark.parametrize("dd", tor.DENSE_DTYPES)
def test_the_dense_index_carries_the_pattern(model, dd, k, mode):
    """S = +0: the order is index_scores_kernel's alone.  33 queries are two dense tiles, the second of one query, and two chunks"""
    for fx in tor.hybrid_dense_fixtures(dd, "f32", k, mode):
        assert pybert.test_hybrid_chunk(fx.n, 33) == (32, (fx.n + 63) // 64 * 64)
        dix, six = pair(model, fx)
        run_layouts(dix, six, fx, k, tor.HYBRID_DENSE_NQS, allow=fx.ok)
        if mode == "allow":
            run_layouts(dix, six, fx, k, tor.HYBRID_DENSE_NQS, allow=fx.ok1, qual=fx.ok1, what="near miss")
        dix.close()
        six.close()


@pytest.mark.parametrize("k", tor.HYBRID_SPARSE_KS)
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
@pytest.mark.parametrize("dd", ["f32", "f16"])
def test_the_sparse_index_carries_the_pattern(model, dd, sd, k):
    """D = +0 against rows that are not zero: the order is the sparse term's alone"""
    fx = tor.hybrid_sparse_fixture(dd, sd, k)
    dix, six = pair(model, fx)
    run_layouts(dix, six, fx, k, tor.HYBRID_NQS)
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# every D the scan reads
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dd", tor.DENSE_DTYPES)
def test_every_dense_score_comes_back_once(model, dd):
    """Weights (1, 0) and allow-lists of 256 consecutive rows, k = 256, 33 queries: every row of the index comes back exactly once with
    H = D + (+-0) — every float of the score matrix that a scan may read, against the reference's D.  The sparse queries hold a term of
    either sign here, so that 0 * S is a zero of either sign; the contract leaves that sign open: scores are compared with ==."""
    k, nq = 256, 33
    for fx in tor.hybrid_dense_fixtures(dd, "f32", k, "plain"):
        lay = tor.layouts(fx.kinds, fx.busy, fx.idle, nq, tile_of(fx, nq, k))["mixed"]
        assert set(lay) == set(fx.kinds)
        dq, _, _ = tor.hybrid_queries(fx, lay)
        q_ids = np.arange(nq, dtype=np.int32)[:, None] % fx.width
        q_w = np.where(np.arange(nq) % 2 == 0, np.float32(1), np.float32(-1))[:, None]
        D = np.stack([fx.dsc[kk] for kk in lay])
        assert not np.isnan(D).any()
        dix, six = pair(model, fx)
        back = []
        for a in range(0, fx.n, k):
            m = min(k, fx.n - a)
            window = np.zeros(fx.n, dtype=bool)
            window[a:a + m] = True
            ids, sc = dix.hybrid_search(six, dq, q_ids, q_w, k, 1.0, 0.0, allow=window)
            for q in range(nq):
                order = np.lexsort((np.arange(m), -D[q, a:a + m].astype(np.float64)))                      # the order rule over the window
                assert np.array_equal(ids[q, :m], a + order) and (ids[q, m:] == -1).all(), (fx.name, a, q, lay[q])
                assert np.array_equal(sc[q, :m], D[q, a + order]) and np.isneginf(sc[q, m:]).all(), (fx.name, a, q, lay[q])
            back.append(ids[:, :m])
        back = np.sort(np.concatenate(back, axis=1), axis=1)
        assert (back == np.arange(fx.n)[None, :]).all(), fx.name
        dix.close()
        six.close()


# ------------------------------------------------------------------------------------------------
# chunks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "allow"])
@pytest.mark.parametrize("sd", tor.SPARSE_DTYPES)
def test_chunks_of_two_queries(model, sd, mode):
    """"hybrid_chunk_queries" = 2 on the sparse index's context: 5 queries are chunks of 2, 2 and 1, each reading the matrix by its
    query's index in the chunk; the results are the unchunked ones"""
    k, nq, pref = tor.HYBRID_CHUNK_K, tor.HYBRID_CHUNK_NQ, tor.HYBRID_CHUNK
    assert pybert.test_hybrid_chunk(tor.SPARSE_ROWS, nq) == (5, 4032) and pybert.test_hybrid_chunk(tor.SPARSE_ROWS, nq, pref) == (2, 4032)
    assert tor.hybrid_chunks(tor.SPARSE_ROWS, nq, pref, pybert.test_hybrid_chunk)[0] == [(0, 2), (2, 2), (4, 1)]
    for w in tor.HYBRID_WEIGHTS:
        fx = tor.hybrid_split_fixture(sd, sd, k, mode, w)
        dix, six = pair(model, fx)
        whole = run_layouts(dix, six, fx, k, (nq,), allow=fx.ok, what="one chunk")
        try:
            model.set_option("hybrid_chunk_queries", str(pref))
            chunked = run_layouts(dix, six, fx, k, (nq,), allow=fx.ok, pref=pref, what="chunks of 2")
        finally:
            model.set_option("hybrid_chunk_queries", "0")
        assert whole.keys() == chunked.keys() and len(whole) >= 3
        for key in whole:
            ixr.assert_same(chunked[key], whole[key], (fx.name, key))
        dix.close()
        six.close()


# ------------------------------------------------------------------------------------------------
# many slices
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(model):
    fx = tor.many_hybrid_fixture()
    dix, six = pair(model, fx)
    yield fx, dix, six
    dix.close()
    six.close()


@pytest.mark.parametrize("k", tor.MANY_KS)
def test_many_slices_read_their_own_rows_scores(model, many, k):
    """17 slices: every slice beats all earlier ones through rows whose D lies beyond the first slice's floats of the query's scores"""
    fx, dix, six = many
    want = tor.hybrid_reference(fx, k)
    assert want["asc"][0][0, 0] == fx.n - 1 and want["desc"][0][0].tolist() == list(range(k)) == want["const"][0][0].tolist()
    for nq in tor.MANY_NQS:
        for c0, c in tor.hybrid_chunks(fx.n, nq, 0, pybert.test_hybrid_chunk)[0]:
            assert pybert.test_sparse_scan_geometry(0, tor.SPARSE_V, fx.n, c, k)["n_slices"] >= 17
        lay = tor.many_layout(nq)
        got = dix.hybrid_search(six, *tor.hybrid_queries(fx, lay), k)
        ixr.assert_same(got, tor.of_layout(want, lay), (fx.name, k, nq))


# ------------------------------------------------------------------------------------------------
# which kernels this file ran
# ------------------------------------------------------------------------------------------------
def test_every_hybrid_kernel_ran_under_this_file(model):
    """a small search per instantiation of its own (so that the test stands alone), then the profiler's launch counts, which after a run
    of the whole file hold every test above"""
    k = 128
    fxs = [tor.hybrid_split_fixture(sd, sd, k, "allow", (1.0, 1.0)) for sd in tor.SPARSE_DTYPES]
    fxs += [tor.hybrid_dense_fixtures(dd, "f32", k, "allow")[0] for dd in ("i8", "b1")]
    for fx in fxs:
        dix, six = pair(model, fx)
        q = tor.hybrid_queries(fx, fx.kinds)
        ixr.assert_same(dix.hybrid_search(six, *q, k), tor.of_layout(tor.hybrid_reference(fx, k, np.ones(fx.n, bool)), fx.kinds), (fx.name, "plain"))
        ixr.assert_same(dix.hybrid_search(six, *q, k, allow=fx.ok), tor.of_layout(tor.hybrid_reference(fx, k), fx.kinds), (fx.name, "masked"))
        dix.close()
        six.close()
    rep = model.profile_report()
    names = [f"sparse_hybrid_scan_{d}{m}" for d in tor.SPARSE_DTYPES for m in ("", "_masked")]
    names += [f"index_scores_{d}{m}" for d in tor.DENSE_DTYPES for m in ("", "_masked")] + ["mask_and", "topk_merge"]
    for name in names:
        print(f"{name}: {rep.get(name, {}).get('launches', 0)} launches")
    for name in names:
        assert rep.get(name, {}).get("launches", 0) >= 1, (name, sorted(rep))
