"""The token index's life cycle on the GPU (include/bert_hip.h "LATE INDEX"): removed documents, allow-lists, rescoring, compaction,
files, capture and bert-search's file flags.  The oracle is the token index's own (test_gpu_token_index.py): S = BertModel.maxsim on
all pairs of the same rows, the columns of documents that do not qualify set to NaN, pushed through token_index_reference's order
rule.  Ids must be equal and scores equal in bits where they are not zero: there is no allowance.

The shapes are the smallest at which the masked scan can go wrong: a mask word is 32 documents, a step of the scan 64, a wave takes
every fourth document of a step — so 1, 31 .. 33, 63 .. 65 documents and 1573 = 64 x 24 + 37, each under 1, 2, 7, n_docs and planned
slices (slices then start inside a mask word and inside a step), and patterns that empty whole steps, whole waves or all but one
document of a step."""
import os
import subprocess

import numpy as np
import pytest

import maxsim_reference as mr
import token_index_file as tf
import token_index_reference as tref
from bert_cpp_amd import pybert
from hip_graph import Hip

from conftest import ROOT
from test_gpu_long_text import text_model  # noqa: F401  (fixture: the `tiny` dims with a vocabulary of real words)
from test_gpu_token_index import LINES, QUERIES

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
N_DOCS = [1, 31, 32, 33, 63, 64, 65, 1573]
KS = [1, 10, 256]


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.set_option("token_index_slices", "0")
    m.close()


_CASES = {}


def _case(model, dim, n):
    """documents, queries and the oracle's score matrix of a (dim, n_docs), made once and left unchanged"""
    if (dim, n) not in _CASES:
        rng = np.random.default_rng(7000 + 13 * dim + n)
        d, dcu = tref.documents(rng, n, dim)
        q, qcu = tref.queries(rng, dim)
        S = model.maxsim(q, qcu, d, dcu)
        assert S.shape == (len(qcu) - 1, n) and np.isfinite(S).all()
        S.setflags(write=False)
        _CASES[(dim, n)] = dict(d=d, dcu=dcu, q=q, qcu=qcu, S=S, n=n, dim=dim)
    return _CASES[(dim, n)]


def _f16(hip, rows):
    return hip.upload(np.ascontiguousarray(rows, dtype=np.float32).astype(np.float16))


def _index(model, c, d_rows=None):
    """the case's documents in a fresh index (from the device copy d_rows where there is one)"""
    ix = model.token_index(c["dim"])
    if d_rows is None:
        assert ix.add(c["d"], c["dcu"]) == 0
    else:
        assert ix.add_device(c["dcu"], d_rows) == 0
    assert len(ix) == c["n"] and ix.n_live() == c["n"] and ix.n_live_tokens() == ix.n_tokens() == int(c["dcu"][-1])
    return ix


def _expected(S, qual, k):
    """the search over the documents qual (bool [n_docs]) alone"""
    Sm = np.array(S, dtype=np.float32)
    Sm[:, ~np.asarray(qual, dtype=bool)] = np.nan
    return tref.search_expected(Sm, k)


def _device_search(hip, ix, q, qcu, max_q_len, k, words=None, stream=0):
    nq = len(qcu) - 1
    d_q, d_qcu = _f16(hip, q), hip.upload(np.asarray(qcu, np.int32))
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    d_w = hip.upload(words) if words is not None else None
    ix.search_device(nq, d_qcu, d_q, max_q_len, k, d_ids, d_sc, stream, d_w, 0 if words is None else len(words))
    out = hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)
    hip.free(d_q, d_qcu, d_ids, d_sc, *([d_w] if d_w else []))
    return out


def patterns(n, rng):
    """name -> bool [n]: the documents that qualify"""
    d = np.arange(n)
    p = {"all ones": np.ones(n, bool), "all zeros": np.zeros(n, bool),
         "one document per step": d % 64 == 5 % max(n, 1),
         "a step cleared between two full ones": ~((d >= 64) & (d < 128)),
         "only the last step": d >= (n - 1) // 64 * 64,
         "alternating": d % 2 == 0,
         "random 50 %": rng.random(n) < 0.5, "random 1 %": rng.random(n) < 0.01}
    for w in range(4):
        p[f"only wave {w}"] = d % 4 == w
    few = np.zeros(n, bool)
    few[rng.choice(n, min(n, 3), replace=False)] = True
    p["fewer than k"] = few
    return p


def _slicings(n):
    return ["1", "2", "7", str(n), "0"]


# ------------------------------------------------------------------------------------------------
# the masked scan: allow-lists, removals, both
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(dim, n) for dim in (8, 64) for n in N_DOCS] + [(384, 130)])
def test_patterns_as_allow_lists_removals_and_both(model, dim, n):
    c = _case(model, dim, n)
    q, qcu, S = c["q"], c["qcu"], c["S"]
    hip = Hip()
    rng = np.random.default_rng(100 + n)
    d_rows = _f16(hip, c["d"])
    plain = _index(model, c, d_rows)
    try:
        for name, qual in patterns(n, rng).items():
            want = {k: _expected(S, qual, k) for k in KS}
            assert (want[256][0] >= 0).sum() == len(S) * min(int(qual.sum()), 256), name
            # "both": live & allow == qual, neither alone equal to it (r splits the documents that do not qualify between the two)
            r = rng.random(n) < 0.5
            removed, both = model.token_index(dim), model.token_index(dim)
            assert removed.add_device(c["dcu"], d_rows) == 0 and both.add_device(c["dcu"], d_rows) == 0
            hip.sync()
            assert removed.remove(np.flatnonzero(~qual)) == int((~qual).sum()) and removed.n_live() == int(qual.sum())
            assert removed.n_live_tokens() == int(np.diff(c["dcu"])[qual].sum()) and len(removed) == n and removed.n_tokens() == int(c["dcu"][-1])
            both.remove(np.flatnonzero(~(qual | r)))
            modes = (("allow", plain, qual), ("removed", removed, None), ("both", both, qual | ~r))
            for slices in _slicings(n):
                model.set_option("token_index_slices", slices)
                for k in KS:
                    for mode, ix, allow in modes:
                        got = ix.search(q, qcu, k, allow=allow)
                        assert tref.same_result(got, want[k]), (name, mode, slices, k)
            model.set_option("token_index_slices", "0")
            # host against device form: under an allow-list, under removals, under both
            words = pybert.allow_words(qual, n)
            mq = plain.max_query_tokens()
            assert tref.same_result(_device_search(hip, plain, q, qcu, mq, 10, words), want[10]), name
            assert tref.same_result(_device_search(hip, removed, q, qcu, mq, 10), want[10]), name
            assert tref.same_result(_device_search(hip, both, q, qcu, mq, 256, pybert.allow_words(qual | ~r, n)), want[256]), name
            # set bits at and beyond size, and words beyond the index's, are ignored
            wide = np.concatenate([words, np.full(3, 0xFFFFFFFF, np.uint32)])
            if n % 32:
                wide[n // 32] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            assert tref.same_result(plain.search(q, qcu, 10, allow=wide), want[10]), name
            assert tref.same_result(_device_search(hip, plain, q, qcu, mq, 10, wide), want[10]), name
            removed.close(); both.close()
        # too few words: refused, outputs untouched
        if n > 32:
            with pytest.raises(ValueError):
                plain.search(q, qcu, 10, allow=np.ones((n + 31) // 32 - 1, np.uint32))
            with pytest.raises(ValueError):
                _device_search(hip, plain, q, qcu, 128, 10, np.ones((n + 31) // 32 - 1, np.uint32))
        # the plain search of the index that was never removed from is the unfiltered one
        assert tref.same_result(plain.search(q, qcu, 10), tref.search_expected(S, 10))
    finally:
        model.set_option("token_index_slices", "0")
        plain.close()
        hip.free(d_rows)


def test_an_index_without_removals_or_allow_list_launches_the_unmasked_scan(model):
    """the profile names the kernel a search launched: the masked instantiation only under a bitmap or an allow-list"""
    c = _case(model, 8, 65)
    ix = _index(model, c)
    model.profile_report()                                              # (a report clears what was recorded before)
    launched = lambda f: (model.profile(True), f(), model.profile(False), set(model.profile_report()))[3]
    names = launched(lambda: ix.search(c["q"], c["qcu"], 10))
    assert "token_index_scan" in names and "token_index_scan_masked" not in names
    names = launched(lambda: ix.search(c["q"], c["qcu"], 10, allow=np.ones(65, bool)))
    assert "token_index_scan_masked" in names and "token_index_scan" not in names
    ix.remove([3])
    names = launched(lambda: ix.search(c["q"], c["qcu"], 10))
    assert "token_index_scan_masked" in names and "token_index_scan" not in names
    assert ix.compact().tolist() == [i for i in range(65) if i != 3]
    names = launched(lambda: ix.search(c["q"], c["qcu"], 10))
    assert "token_index_scan" in names and "token_index_scan_masked" not in names
    ix.close()


# ------------------------------------------------------------------------------------------------
# remove: refusals, rescore, later adds, get_doc
# ------------------------------------------------------------------------------------------------
def test_remove_counts_refuses_and_rescore_skips_removed_ids(model):
    c = _case(model, 64, 1573)
    q, qcu, S, n = c["q"], c["qcu"], c["S"], c["n"]
    nq = len(qcu) - 1
    hip = Hip()
    ix = _index(model, c)
    rng = np.random.default_rng(21)
    gone = rng.choice(n, 700, replace=False)
    assert ix.remove(gone[:400]) == 400 and ix.remove(np.concatenate([gone[300:], gone[:5], gone[-5:]])) == 300      # repeats, removed ids
    assert ix.remove([]) == 0 and ix.n_live() == n - 700 and len(ix) == n
    for bad in ([n], [-1], [0, n + 7]):
        with pytest.raises(ValueError):
            ix.remove(bad)
    assert ix.n_live() == n - 700
    live = np.ones(n, bool)
    live[gone] = False
    assert np.array_equal(ix.live_ids(), np.flatnonzero(live))
    Sm = np.array(S)
    Sm[:, ~live] = np.nan
    for n_cand in (1, 33, 1024):
        cand = rng.integers(-1, n, (nq, n_cand)).astype(np.int32)
        cand[0, 0] = gone[0]
        for k in KS:
            want = tref.rescore_expected(Sm, cand, k)
            assert tref.same_result(ix.rescore(q, qcu, cand, k), want), (n_cand, k)
            d_q, d_qcu, d_c = _f16(hip, q), hip.upload(qcu), hip.upload(cand)
            d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
            ix.rescore_device(nq, d_qcu, d_q, n_cand, d_c, k, d_ids, d_sc)
            got = hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)
            hip.free(d_q, d_qcu, d_c, d_ids, d_sc)
            assert tref.same_result(got, want), (n_cand, k)
    # only removed candidates: nothing
    got = ix.rescore(q, qcu, np.tile(gone[:8].astype(np.int32), (nq, 1)), 4)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    # a removed document is still read back; search_texts' route (search_device_to_host) is the search's
    for doc in gone[:3]:
        want = c["d"][c["dcu"][doc]:c["dcu"][doc + 1]].astype(np.float16).astype(np.float32)
        assert np.array_equal(ix.get_doc(int(doc)).view(np.uint32), want.view(np.uint32))
    ix.close()


def test_removals_at_the_ends_of_a_word_in_seventy_documents(model):
    """the first and last bit of word 0, the first of word 1 and the index's last document, in the smallest index that has them"""
    rng = np.random.default_rng(7070)
    n, dim, k, gone = 70, 8, 8, [0, 31, 32, 69]
    d, dcu = tref.documents(rng, n, dim, lens=[2, 3, 4, 5])
    q, qcu = tref.queries(rng, dim, lens=[1, 3, 5])
    # what is about to go leads every answer: documents 0 and 32 (2 tokens) start with query 0's token, 69 (3 tokens) is query 1, 31 (5) query 2
    d = np.array(d)
    d[dcu[0]] = d[dcu[32]] = q[0]
    d[dcu[69]:dcu[70]] = q[qcu[1]:qcu[2]]
    d[dcu[31]:dcu[32]] = q[qcu[2]:qcu[3]]
    S = model.maxsim(q, qcu, d, dcu)
    assert S.shape == (3, n) and np.isfinite(S).all()
    ix = model.token_index(dim)
    assert ix.add(d, dcu) == 0
    first = ix.search(q, qcu, 2)[0]
    assert sorted(first[0].tolist()) == [0, 32] and first[1:, 0].tolist() == [69, 31]
    assert ix.remove(gone) == 4 and len(ix) == n and ix.n_live() == n - 4
    assert ix.n_live_tokens() == int(dcu[-1]) - int(np.diff(dcu)[gone].sum())
    live = np.ones(n, bool)
    live[gone] = False
    got = ix.search(q, qcu, k)
    assert not np.isin(got[0], gone).any() and (got[0] >= 0).all()
    assert tref.same_result(got, _expected(S, live, k))
    assert np.array_equal(ix.live_ids(), np.flatnonzero(live))
    ix.close()


def test_a_dense_searchs_ids_rescored_after_a_remove_never_show_the_removed_document(model):
    c = _case(model, 64, 65)
    q, qcu, n = c["q"], c["qcu"], c["n"]
    nq = len(qcu) - 1
    hip = Hip()
    rng = np.random.default_rng(22)
    tix = _index(model, c)
    dense = model.index(32, "f32")
    dense.add(mr.unit_rows(rng, n, 32))
    dq = mr.unit_rows(rng, nq, 32)
    cand, _ = dense.search(dq, 20)
    gone = np.unique(cand[:, :3])                                       # every query's three best dense candidates
    tix.remove(gone)
    d_dq, d_cand, d_csc = hip.upload(dq), hip.nans((nq, 20), np.int32), hip.nans((nq, 20), np.float32)
    d_q, d_qcu = _f16(hip, q), hip.upload(qcu)
    d_ids, d_sc = hip.nans((nq, 10), np.int32), hip.nans((nq, 10), np.float32)
    s = hip.stream()
    dense.search_device(nq, d_dq, 20, d_cand, d_csc, s)
    tix.rescore_device(nq, d_qcu, d_q, 20, d_cand, 10, d_ids, d_sc, s)
    got = hip.download(d_ids, (nq, 10), np.int32), hip.download(d_sc, (nq, 10), np.float32)
    assert not np.isin(got[0], gone).any() and (got[0] >= 0).any()
    Sm = np.array(c["S"])
    Sm[:, gone] = np.nan
    assert tref.same_result(got, tref.rescore_expected(Sm, cand, 10))
    hip.destroy_stream(s)
    hip.free(d_dq, d_cand, d_csc, d_q, d_qcu, d_ids, d_sc)
    dense.close(); tix.close()


def test_documents_added_after_a_remove_are_live_and_found(model):
    c = _case(model, 64, 1573)
    q, qcu, S, d, dcu = c["q"], c["qcu"], c["S"], c["d"], c["dcu"]
    first = 40                                                          # 40 documents, one removed, then the rest in two adds: the
    ix = model.token_index(64)                                          # storage and the bitmap grow past their first capacities
    assert ix.add(d[:dcu[first]], dcu[:first + 1]) == 0
    assert ix.remove([7, 39]) == 2
    assert ix.add(d[dcu[first]:dcu[1100]], dcu[first:1101] - dcu[first]) == first
    assert ix.add(d[dcu[1100]:], dcu[1100:] - dcu[1100]) == 1100
    live = np.ones(1573, bool)
    live[[7, 39]] = False
    assert ix.n_live() == 1571 and len(ix) == 1573 and ix.n_live_tokens() == int(np.diff(dcu)[live].sum())
    for k in (10, 256):
        assert tref.same_result(ix.search(q, qcu, k), _expected(S, live, k)), k
    assert np.array_equal(ix.live_ids(), np.flatnonzero(live))
    # a refused add leaves the bitmap as it was
    with pytest.raises(ValueError):
        ix.add(d, [0, 0, 3])
    assert ix.n_live() == 1571 and tref.same_result(ix.search(q, qcu, 10), _expected(S, live, 10))
    ix.close()


# ------------------------------------------------------------------------------------------------
# compact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(8, 65), (64, 1573), (384, 130)])
def test_compact_keeps_order_bits_and_results(model, dim, n):
    c = _case(model, dim, n)
    q, qcu, S, d, dcu = c["q"], c["qcu"], c["S"], c["d"], c["dcu"]
    rng = np.random.default_rng(30 + n)
    ix = _index(model, c)
    # without removals: the identity
    assert np.array_equal(ix.compact(), np.arange(n)) and len(ix) == n and ix.n_tokens() == int(dcu[-1])
    assert tref.same_result(ix.search(q, qcu, 10), tref.search_expected(S, 10))
    live = rng.random(n) < 0.6
    live[0], live[n - 1] = False, True
    ix.remove(np.flatnonzero(~live))
    before = {k: ix.search(q, qcu, k) for k in (10, 256)}
    assert all(tref.same_result(before[k], _expected(S, live, k)) for k in before)
    docs_before = {int(o): ix.get_doc(int(o)) for o in np.flatnonzero(live)}
    old = ix.compact()
    nl = int(live.sum())
    assert np.array_equal(old, np.flatnonzero(live)) and len(ix) == nl == ix.n_live()
    assert ix.n_tokens() == ix.n_live_tokens() == int(np.diff(dcu)[live].sum())
    for new, o in enumerate(old):
        assert np.array_equal(ix.get_doc(new).view(np.uint32), docs_before[int(o)].view(np.uint32)), new
    for slices in ("0", "7"):
        model.set_option("token_index_slices", slices)
        for k in before:
            got = ix.search(q, qcu, k)
            mapped = np.where(got[0] >= 0, old[np.maximum(got[0], 0)], -1).astype(np.int32)
            assert tref.same_result((mapped, got[1]), before[k]), (slices, k)
    model.set_option("token_index_slices", "0")
    # add after compact; a second compact after more removals
    assert ix.add(d[:dcu[2]], dcu[:3]) == nl and len(ix) == nl + 2
    S2 = np.concatenate([S[:, live], S[:, :2]], axis=1)
    assert tref.same_result(ix.search(q, qcu, 256), tref.search_expected(S2, 256))
    ix.remove([nl])
    keep = np.ones(nl + 2, bool)
    keep[nl] = False
    assert np.array_equal(ix.compact(), np.flatnonzero(keep))
    assert tref.same_result(ix.search(q, qcu, 256), tref.search_expected(S2[:, keep], 256))
    ix.close()


def test_compact_of_an_all_removed_index_gives_an_empty_searchable_index(model):
    c = _case(model, 8, 65)
    ix = _index(model, c)
    assert ix.remove(np.arange(65)) == 65 and ix.n_live() == 0 and ix.n_live_tokens() == 0
    got = ix.search(c["q"], c["qcu"], 5)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    assert len(ix.compact()) == 0 and len(ix) == 0 and ix.n_tokens() == 0
    got = ix.search(c["q"], c["qcu"], 5)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    assert ix.add(c["d"], c["dcu"]) == 0 and tref.same_result(ix.search(c["q"], c["qcu"], 10), tref.search_expected(c["S"], 10))
    ix.close()


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------
def _answers(ix, c, live, rng):
    """search, filtered search and rescore of an index, for a comparison in bits"""
    n = len(live)
    allow = rng.random(n) < 0.5
    cand = rng.integers(-1, max(n, 1), (len(c["qcu"]) - 1, 33)).astype(np.int32) if n else np.full((len(c["qcu"]) - 1, 33), -1, np.int32)
    return [ix.search(c["q"], c["qcu"], 256), ix.search(c["q"], c["qcu"], 10, allow=allow), ix.rescore(c["q"], c["qcu"], cand, 10)]


@pytest.mark.parametrize("dim,n,removals", [(8, 65, True), (8, 65, False), (64, 1573, True), (384, 130, True), (8, 0, False)])
def test_save_and_load(model, tmp_path, dim, n, removals):
    c = _case(model, dim, max(n, 1))
    d, dcu = (c["d"], c["dcu"]) if n else (np.zeros((0, dim), np.float32), np.zeros(1, np.int32))
    ix = model.token_index(dim)
    if n:
        ix.add(d, dcu)
    live = np.ones(n, bool)
    if removals:
        live = np.random.default_rng(40 + n).random(n) < 0.7
        ix.remove(np.flatnonzero(~live))
    path = str(tmp_path / "ix.tok")
    ix.save(path)
    data = open(path, "rb").read()
    # the file's bytes are the Python writer's for the same documents and removals
    assert data == tf.write(d, dcu, live if removals else None)
    assert not os.path.exists(path + ".tmp")
    f = tf.parse(data)
    assert (f["dim"], f["n_docs"], f["has_live"], f["n_tokens"]) == (dim, n, int(removals), int(dcu[-1]))
    written = str(tmp_path / "py.tok")
    open(written, "wb").write(tf.write(d, dcu, live if removals else None))
    Sm = np.array(c["S"][:, :n])
    Sm[:, ~live] = np.nan
    want = _answers(ix, c, live, np.random.default_rng(5))
    assert tref.same_result(want[0], tref.search_expected(Sm, 256))
    for p in (path, written):
        back = model.load_token_index(p)
        assert back.dim == dim and len(back) == n and back.n_tokens() == int(dcu[-1]) and back.n_live() == int(live.sum())
        assert back.n_live_tokens() == ix.n_live_tokens()
        got = _answers(back, c, live, np.random.default_rng(5))
        assert all(tref.same_result(g, w) for g, w in zip(got, want)), p
        # a loaded index goes on living: a save gives the same bytes, an add is found
        again = str(tmp_path / "again.tok")
        back.save(again)
        assert open(again, "rb").read() == data
        if n:
            assert back.add(d[:dcu[1]], dcu[:2]) == n and back.n_live() == int(live.sum()) + 1
            assert np.array_equal(back.get_doc(n).view(np.uint32), back.get_doc(0).view(np.uint32))
        back.close()
    ix.close()


def test_a_loaded_index_of_another_dim_refuses_the_text_routes(model, tmp_path):
    c = _case(model, 8, 65)
    assert model.n_embd != 8
    ix = _index(model, c)
    path = str(tmp_path / "dim8.tok")
    ix.save(path)
    back = model.load_token_index(path)
    with pytest.raises(ValueError):
        back.add_texts(["hello"])
    with pytest.raises(ValueError):
        back.search_texts(["hello"], 3)
    assert len(back) == 65
    back.close(); ix.close()


def test_damaged_files_are_refused_with_a_message(model, tmp_path, capfd):
    """every check stands in front of the index's creation, so a refused file leaves nothing behind; the context goes on working"""
    c = _case(model, 8, 65)
    live = np.ones(65, bool)
    live[[3, 64]] = False
    good = tf.write(c["d"], c["dcu"], live)
    cu_at = lambda i: 64 + 4 * i
    put = lambda data, at, v: data[:at] + int(v & 0xFFFFFFFF).to_bytes(4, "little") + data[at + 4:]
    cu7, cu6, last = int(c["dcu"][7]), int(c["dcu"][6]), int(c["dcu"][65])
    live_at = 64 + 66 * 4 + last * 16
    bad = {"truncated": good[:-1], "header only": good[:64], "half a header": good[:30], "empty": b"",
           "appended": good + b"\0", "appended words": good + b"\0" * 4,
           "cu[0] = 1": put(good, cu_at(0), 1), "an equal pair": put(good, cu_at(7), cu6), "a descent": put(good, cu_at(7), cu6 - 1),
           "a negative entry": put(good, cu_at(7), -5), "last != n_tokens": put(good, cu_at(65), last - 1),
           "a live bit at n_docs": good[:live_at + 8] + bytes([good[live_at + 8] | 0x02]) + good[live_at + 9:],
           "wrong magic": b"BHIPSPX1" + good[8:], "dim 12": put(good, 12, 12)}
    assert cu7 > cu6
    for name, data in bad.items():
        p = tmp_path / "bad.tok"
        p.write_bytes(data)
        capfd.readouterr()
        assert not model.lib.bert_hip_late_index_load(model.ctx, os.fsencode(str(p))), name
        err = capfd.readouterr().err
        assert "bert_hip_late_index_load: '" in err and len(err.strip().splitlines()) == 1, (name, err)
        with pytest.raises(RuntimeError):
            model.load_token_index(str(p))
    capfd.readouterr()
    assert not model.lib.bert_hip_late_index_load(model.ctx, os.fsencode(str(tmp_path / "missing.tok")))
    assert "cannot read" in capfd.readouterr().err
    # the good file loads, and answers
    p = tmp_path / "good.tok"
    p.write_bytes(good)
    back = model.load_token_index(str(p))
    assert tref.same_result(back.search(c["q"], c["qcu"], 10), _expected(c["S"], live, 10))
    with pytest.raises(ValueError):
        back.save("")
    back.close()


# ------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------
def test_the_filtered_search_is_captured_and_a_later_remove_is_seen_by_the_replay(model):
    c = _case(model, 64, 1573)
    q, qcu, S, n = c["q"], c["qcu"], c["S"], c["n"]
    nq, k = len(qcu) - 1, 10
    hip = Hip()
    ix = model.token_index(64)
    ix.reserve(n, int(c["dcu"][-1]), nq, 128, k)
    assert ix.add(c["d"], c["dcu"]) == 0
    rng = np.random.default_rng(50)
    allow = rng.random(n) < 0.5
    live = np.ones(n, bool)
    live[:3] = False
    ix.remove([0, 1, 2])                                                # the bitmap exists before the capture
    words = pybert.allow_words(allow, n)
    d_q, d_qcu, d_w = _f16(hip, q), hip.upload(qcu), hip.upload(words)
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    s = hip.stream()
    read = lambda: (hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32))
    ix.search_device(nq, d_qcu, d_q, 128, k, d_ids, d_sc, s, d_w, len(words))
    eager = read()
    assert tref.same_result(eager, _expected(S, live & allow, k))
    with hip.capture(s) as cap:
        ix.search_device(nq, d_qcu, d_q, 128, k, d_ids, d_sc, s, d_w, len(words))
    assert cap.status == 0 and cap.graph and hip.kernel_nodes(cap.graph) == 2          # the masked scan, the merge
    ex = hip.instantiate(cap.graph)
    hip.poison(d_ids, (nq, k), np.int32); hip.poison(d_sc, (nq, k), np.float32)
    hip.launch(ex, s)
    replay = read()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(replay, eager))
    # a remove between two replays: the words are updated in place, the second replay sees it
    best = np.unique(eager[0][:, 0])
    assert ix.remove(best) == len(best)
    live[best] = False
    hip.poison(d_ids, (nq, k), np.int32); hip.poison(d_sc, (nq, k), np.float32)
    hip.launch(ex, s)
    second = read()
    assert not np.isin(second[0], best).any() and tref.same_result(second, _expected(S, live & allow, k))
    # and a change of the caller's own words
    allow[:] = True
    hip.write(d_w, pybert.allow_words(allow, n))
    hip.launch(ex, s)
    assert tref.same_result(read(), _expected(S, live, k))
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qcu, d_w, d_ids, d_sc)
    ix.close()


# ------------------------------------------------------------------------------------------------
# the example
# ------------------------------------------------------------------------------------------------
def test_bert_search_saves_and_loads_the_token_index(text_model, tmp_path):
    path, _ = text_model
    lines = [l for l in LINES if l]
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    tok = str(tmp_path / "lines.tok")
    exe = os.path.join(BIN, "bert-search")
    stdin = "".join(q + "\n" for q in QUERIES) + "q\n"
    run = lambda flags: subprocess.run([exe, "-m", path, "-f", str(f), "-k", "3"] + flags, input=stdin, capture_output=True, text=True, timeout=300)
    plain, saved = run(["--late"]), run(["--late", "--save-tokens", tok])
    assert plain.returncode == 0 and saved.returncode == 0, (plain.stderr, saved.stderr)
    assert plain.stdout.count("MaxSim score") == 3 * len(QUERIES) and saved.stdout == plain.stdout
    loaded = run(["--late", "--load-tokens", tok])
    assert loaded.returncode == 0 and loaded.stdout == plain.stdout, loaded.stderr
    # the same file serves --maxsim N --token-index
    kept, from_file = run(["--maxsim", "20", "--token-index"]), run(["--maxsim", "20", "--token-index", "--load-tokens", tok])
    assert kept.returncode == 0 and from_file.returncode == 0 and from_file.stdout == kept.stdout, from_file.stderr
    # the file is the binding's, and a TEXTS of another length is an error
    m = pybert.BertModel(path)
    ix = m.token_index()
    ix.add_texts(lines)
    ix.save(str(tmp_path / "py.tok"))
    assert open(tok, "rb").read() == open(tmp_path / "py.tok", "rb").read()
    ix.close(); m.close()
    f.write_text("\n".join(lines[:-1]) + "\n")
    short = run(["--late", "--load-tokens", tok])
    assert short.returncode == 1 and "documents" in short.stderr
