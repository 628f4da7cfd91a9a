"""The grouped scan of the f16 token index (token_index_grouped.hip; the tuning key "token_index_query_group"): G consecutive queries a
workgroup, every document block read once per group.  The oracle is the f16 index's own: BertModel.maxsim on all pairs pushed through
the order rule (token_index_reference.py) — ids equal, score bits equal — and the float64 bound of maxsim_reference.  The ordered
fixtures are topk_order_reference.py's token fixtures, whose scores are exact."""
import numpy as np
import pytest

import maxsim_reference as mr
import token_index_reference as tref
import topk_order_reference as tor
from bert_cpp_amd import pybert
from hip_graph import Hip

from test_gpu_token_index import N_DOCS, _device_search, _f16, _hold_f64, _index

gpu = pytest.mark.gpu
_DOCS = {}


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.set_option("token_index_query_group", "0")
    m.set_option("token_index_slices", "0")
    m.close()


def _docs(dim):
    if dim not in _DOCS:
        _DOCS[dim] = tref.documents(np.random.default_rng(7000 + dim), N_DOCS, dim)
    return _DOCS[dim]


def _case(model, dim, lens):
    """the dim's 300 documents, queries of these lengths and the oracle's matrix"""
    d, dcu = _docs(dim)
    q, qcu, _ = mr.packed_set(np.random.default_rng(dim + len(lens)), lens, dim)
    return dict(d=d, dcu=dcu, q=q, qcu=np.asarray(qcu, np.int32), S=model.maxsim(q, qcu, d, dcu))


def _group(dim, max_q_len, nq, k, key):
    """token_index_kernels.h token_query_group for key >= 1, restated: the largest G <= 4, nq, key whose blocks and lists fit the LDS"""
    fits = lambda g: g * (-(-max_q_len // 32) * 64 * (dim + 8) + 8 * tor.token_L(k)) + 16 <= 160 * 1024 - 256
    return max([g for g in range(1, min(4, nq, key) + 1) if fits(g)] or [1])


def _launched(model, f):
    model.profile_report()
    model.profile(True)
    got = f()
    model.profile(False)
    return got, set(model.profile_report())


def test_the_hook_against_its_restatement():
    for dim in (8, 384, 768, 1024):
        for mql in (m for m in (1, 32, 33, 128) if m <= tref.max_query_tokens(dim)):
            for k in (10, 256):
                for nq in (1, 2, 3, 5):
                    for key in (1, 2, 3, 4):
                        assert pybert.test_late_index_query_group(dim, 1, mql, nq, k, key) == _group(dim, mql, nq, k, key), (dim, mql, k, nq, key)
                    planned = pybert.test_late_index_query_group(dim, 1, mql, nq, k, 0)
                    assert 1 <= planned <= _group(dim, mql, nq, k, 4) and (nq > 1 or planned == 1)
                    assert pybert.test_late_index_query_group(dim, 2, mql, nq, k, 4) == pybert.test_late_index_query_group(dim, 4, mql, nq, k, 4) == 1
    assert [_group(d, 32, 9, 10, 4) for d in (384, 768, 1024)] == [4, 3, 2] and _group(384, 128, 9, 10, 4) == 1
    assert pybert.test_late_index_query_group(384, 1, 32, 4, 10, 5) is None and pybert.test_late_index_query_group(384, 1, 129, 4, 10, 0) is None


@gpu
@pytest.mark.parametrize("dim,lens,key,G", [(8, [1, 31, 32, 7, 32], 4, 4), (24, [32] * 7, 4, 4), (384, [33, 64, 1], 2, 2), (768, [32, 5, 17, 32], 0, None),
                                            (768, [32, 5, 17, 32], 3, 3), (1024, [32, 32, 9], 2, 2)])
def test_shapes_against_the_oracle(model, dim, lens, key, G):
    c = _case(model, dim, lens)
    f64 = tref.scores_f64(c["q"], c["qcu"], c["d"], c["dcu"])
    ix = _index(model, dim, c["d"], c["dcu"])
    model.set_option("token_index_query_group", str(key))
    for k in (1, 10, 256):
        hook = pybert.test_late_index_query_group(dim, 1, max(lens), len(lens), k, key)
        # (key 0: what the measured plan gives, within the rule's bound)
        assert hook == (G or hook) and 1 <= hook <= _group(dim, max(lens), len(lens), k, 4), (dim, k, hook)
        got, names = _launched(model, lambda: ix.search(c["q"], c["qcu"], k))
        assert ("token_index_scan_grouped" in names) == (hook >= 2) and ("token_index_scan" in names) == (hook < 2), (dim, key, k, names)
        assert tref.same_result(got, tref.search_expected(c["S"], k)), (dim, key, k)
        _hold_f64(got, f64, f"grouped dim {dim} key {key}")
    ix.close()


@gpu
@pytest.mark.parametrize("dim", [24, 384])
def test_a_result_depends_on_neither_key(model, dim):
    """queries of up to 64 tokens: G = 1, 2, 3, 4 under the keys at dim 24 and 1, 2, 3, 3 at dim 384 (the LDS)"""
    c = _case(model, dim, [32, 5, 33, 64, 1, 17, 20])
    q, qcu = c["q"], c["qcu"]
    nq, k = len(qcu) - 1, 256
    want = tref.search_expected(c["S"], k)
    hip = Hip()
    ix = model.token_index(dim)
    ix.reserve(N_DOCS, int(c["dcu"][-1]), nq, 64, k)
    assert ix.add(c["d"], c["dcu"]) == 0
    for key in (1, 2, 3, 4):
        model.set_option("token_index_query_group", str(key))
        for slices in (0, 1, 7, N_DOCS):
            model.set_option("token_index_slices", str(slices))
            assert tref.same_result(ix.search(q, qcu, k), want), (key, slices)
    # host against device entry point, then captured and replayed within reserve (key 4, the planned slices)
    model.set_option("token_index_slices", "0")
    assert tref.same_result(_device_search(hip, ix, q, qcu, 64, k), want)
    d_q, d_qcu, d_ids, d_sc = _f16(hip, q), hip.upload(qcu), hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    s = hip.stream()
    with hip.capture(s) as cap:
        ix.search_device(nq, d_qcu, d_q, 64, k, d_ids, d_sc, s)
    assert cap.status == 0 and cap.graph and hip.kernel_nodes(cap.graph) == 2                 # scan, merge
    ex = hip.instantiate(cap.graph)
    for _ in range(2):
        hip.poison(d_ids, (nq, k), np.int32); hip.poison(d_sc, (nq, k), np.float32)
        hip.launch(ex, s)
        assert tref.same_result((hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)), want)
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qcu, d_ids, d_sc)
    model.set_option("token_index_slices", "0")
    ix.close()


@gpu
def test_guards_inside_a_group(model):
    """eight queries, key 4: 5 tokens | empty | 40 tokens, longer than max_q_len 32 | descending (45 -> 40) | 20 | 10 | 20 | 10 tokens"""
    c = _case(model, 64, [100])
    rows, qcu = c["q"], np.array([0, 5, 5, 45, 40, 60, 70, 90, 100], np.int32)
    good = [0, 4, 5, 6, 7]
    gcu = np.concatenate([[0], np.cumsum([qcu[i + 1] - qcu[i] for i in good])]).astype(np.int32)
    S = model.maxsim(np.concatenate([rows[qcu[i]:qcu[i + 1]] for i in good]), gcu, c["d"], c["dcu"])
    ix = _index(model, 64, c["d"], c["dcu"])
    model.set_option("token_index_query_group", "4")
    got = _device_search(Hip(), ix, rows, qcu, 32, 6)
    for bad in (1, 2, 3):
        assert (got[0][bad] == -1).all() and np.isneginf(got[1][bad]).all(), bad
    assert tref.same_result((got[0][good], got[1][good]), tref.search_expected(S, 6))
    ix.close()


@gpu
def test_masked_groups(model):
    """every third document removed, a random allow-list, together and apart; documents 64 .. 127 — one step of one slice — all masked"""
    c = _case(model, 64, [32, 1, 31, 32, 9, 32])
    rng = np.random.default_rng(3)
    live, allow = np.arange(N_DOCS) % 3 != 0, rng.random(N_DOCS) < 0.5
    allow[64:128] = False
    plain, removed = _index(model, 64, c["d"], c["dcu"]), _index(model, 64, c["d"], c["dcu"])
    assert removed.remove(np.flatnonzero(~live)) == int((~live).sum())
    model.set_option("token_index_query_group", "4")
    for slices in (1, 7):
        model.set_option("token_index_slices", str(slices))
        for ix, words, qual in ((removed, None, live), (plain, allow, allow), (removed, allow, live & allow)):
            Sm = c["S"].copy()
            Sm[:, ~qual] = np.nan
            for k in (10, 256):
                got, names = _launched(model, lambda: ix.search(c["q"], c["qcu"], k, allow=words))
                assert names >= {"token_index_scan_grouped_masked"} and tref.same_result(got, tref.search_expected(Sm, k)), (slices, k)
    model.set_option("token_index_slices", "0")
    plain.close(); removed.close()


@gpu
@pytest.mark.parametrize("k", [1, 192, 193, 256])
def test_selection_with_four_lists(model, k):
    """ascending, descending, constant and the exact-fit staircase of this k over the same documents, one group: one slice and 17"""
    fx = tor.token_fixture(k)
    kinds = ["asc", "desc", "const", "stair"]
    q, qcu = tor.token_queries(kinds, [1] * 4)
    want = tor.reference_topk(np.stack([fx.scores[kk] for kk in kinds]), True, k)
    ix = _index(model, tor.TOKEN_DIM, fx.rows, fx.cu)
    model.set_option("token_index_query_group", "4")
    for slices in (1, 17):
        model.set_option("token_index_slices", str(slices))
        got, names = _launched(model, lambda: ix.search(q, qcu, k))
        assert "token_index_scan_grouped" in names and tref.same_result(got, want), (k, slices)
    model.set_option("token_index_slices", "0")
    ix.close()


@gpu
def test_a_chunk_and_one_query_in_groups_of_three(model):
    """257 one-token queries at dim 768 (G = 3: 85 groups and one query in the chunk of 256, then a chunk of one), row for row"""
    d, dcu = _docs(768)
    q = mr.unit_rows(np.random.default_rng(11), 257, 768)
    ix = _index(model, 768, d, dcu)
    model.set_option("token_index_query_group", "4")
    got = ix.search(q, np.arange(258, dtype=np.int32), 10)
    alone = [ix.search(q[i:i + 1], [0, 1], 10) for i in range(257)]
    assert tref.same_result(got, (np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone])))
    ix.close()
