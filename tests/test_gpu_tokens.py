"""Token rows out of the forward pass and MaxSim scoring (include/bert_hip.h "token rows and late interaction") on the GPU: the
copy kernel at op level, the token-rows pass end to end (the tiled and generic kernels of the small models in f16 and q4_0, the f32
route, the fused route of a batch the one-launch kernel would have taken), the host form's chunking, the MaxSim kernel
against the float64 reference within its derived bound (maxsim_reference.py), its masking, its bit rules and its error cases, and
bert-search --maxsim.  The worst fraction of each bound is recorded in _WORST and printed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import maxsim_reference as mr
from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

from conftest import ROOT
from test_gpu_long_text import text_model  # noqa: F401  (fixture: the `tiny` dims with a vocabulary of real words)
from test_gpu_pooling import _Hip, _cu, _set_mode

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
_WORST = {}


def _hold(got, want, bound, what):
    """|got - want| <= bound everywhere; prints (and records) the worst fraction of the bound"""
    got = np.asarray(got)
    err = np.abs(got.astype(np.float64) - want)
    pos = bound > 0
    frac = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    _WORST[what] = max(_WORST.get(what, 0.0), frac)
    print(f"{what}: worst fraction of the bound {frac:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, frac)
    return frac


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ------------------------------------------------------------------------------------------------
# the token-row kernel, through bert_hip_test_token_rows
# ------------------------------------------------------------------------------------------------
ROW_LENS = [1, 2, 31, 33, 128]
F16_NAN, F32_NAN = 0x7E00, 0x7FC00000


@pytest.mark.parametrize("src", ["f16", "f32"])
@pytest.mark.parametrize("H", [8, 64, 130, 384, 768])
def test_token_rows_kernel(H, src):
    """Every flag combination on both stored types, NaNs behind the last token and in the output beforehand: normalised rows against
    float64 within gamma(H + 2) (plus the f16 rounding), un-normalised f32 rows the stored values bit for bit."""
    rng = np.random.default_rng(H)
    cu = _cu(ROW_LENS)
    x = rng.normal(0.1, 1, (int(cu[-1]), H)).astype(np.float16 if src == "f16" else np.float32)
    with pybert.test_pad(F16_NAN, F32_NAN):
        for normalize in (False, True):
            for f16_out in (False, True):
                got = pybert.test_token_rows(x, cu, 128, normalize, f16_out)
                assert got.dtype == (np.float16 if f16_out else np.float32) and got.shape == x.shape
                want, bound = mr.token_rows_reference(x, normalize, f16_out)
                _hold(got, want, bound, f"token_rows {src} H {H} normalize {int(normalize)} f16 {int(f16_out)}")
                if not normalize and not f16_out:
                    assert np.array_equal(_bits(got), _bits(x.astype(np.float32)))
                if normalize and not f16_out:
                    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-5
        # a sentence over max_len: NaN rows for its tokens, and for them only
        for f16_out in (False, True):
            got = pybert.test_token_rows(x, cu, 64, True, f16_out)
            assert np.isnan(got[cu[4]:cu[5]]).all() and np.isfinite(got[:cu[4]]).all()
            assert np.array_equal(_bits(got[:cu[4]]), _bits(pybert.test_token_rows(x, cu, 128, True, f16_out)[:cu[4]]))


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
E2E_LENS = [1, 2, 3, 17, 31, 32, 33, 48, 64]
E2E_MODELS = [(d, f) for d in ("tiny", "tiny-d64", "tiny-h128", "tiny-d16") for f in ("f16", "q4_0")] + [("tiny", "f32")]
# test_hidden_states_match_oracle's tolerance per layer (f32: test_gpu_pooling.py's HIDDEN_TOL, from test_f32_route_hidden_states)
HIDDEN_TOL = {"f16": 6e-3, "q4_0": 0.25, "f32": 2e-4}


def _batch(hp, seed=300):
    sents = [gf.synthetic_token_ids(1, min(n, hp.n_max_tokens), hp.n_vocab, seed=seed + i)[0] for i, n in enumerate(E2E_LENS)]
    return sents, np.concatenate(sents).astype(np.int32), _cu([len(s) for s in sents])


@pytest.mark.parametrize("dims,ftype", E2E_MODELS)
def test_token_rows_end_to_end(make_model, dims, ftype):
    path, hp = make_model(dims, ftype, 2)
    m = pybert.BertModel(path)
    sents, toks, cu = _batch(hp)
    # cls, un-normalised: the first token's row IS the embedding, the call's own and a separate eval_packed call's
    _set_mode(m, ("cls", "0"))
    rows, emb = m.eval_packed_tokens(toks, cu, normalize=False, with_embeddings=True)
    plain = m.eval_packed(toks, cu)
    assert np.isfinite(rows).all() and rows.shape == (int(cu[-1]), hp.n_embd)
    for s in range(len(sents)):
        assert np.array_equal(_bits(rows[cu[s]]), _bits(emb[s])) and np.array_equal(_bits(rows[cu[s]]), _bits(plain[s])), (dims, ftype, s)
    # mean, un-normalised: the float64 mean of a sentence's rows against its embedding, within test_gpu_pooling.py's pooling bound
    _set_mode(m, ("mean", "0"))
    rows_m, emb_m = m.eval_packed_tokens(toks, cu, normalize=False, with_embeddings=True)
    assert np.array_equal(_bits(rows_m), _bits(rows))                       # (the rows do not depend on the pooling mode)
    assert np.array_equal(_bits(emb_m), _bits(m.eval_packed(toks, cu)))
    for s in range(len(sents)):
        want = rows[cu[s]:cu[s + 1]].astype(np.float64).mean(axis=0)
        _hold(emb_m[s], want, np.full(want.shape, 2e-6 * max(1.0, float(np.abs(want).max()))), f"mean of rows {dims} {ftype}")
    # the oracle's last hidden layer
    o = orc.Oracle(path)
    tol = HIDDEN_TOL[ftype] * (1 + hp.n_layer)
    for s, ids in enumerate(sents):
        want = o.eval(ids, orc.MODE_PLAIN, want_hidden=True)[1][-1].astype(np.float64)
        _hold(rows[cu[s]:cu[s + 1]], want, np.full(want.shape, tol), f"oracle hidden {dims} {ftype}")
    # a sentence's rows: the same bits alone and inside the batch; normalised rows: the un-normalised ones over their norm
    unit = m.eval_packed_tokens(toks, cu, normalize=True)
    want, bound = mr.token_rows_reference(rows, True, False)
    _hold(unit, want, bound, f"normalised rows {dims} {ftype}")
    for s, ids in enumerate(sents):
        alone = m.eval_packed_tokens(ids, _cu([len(ids)]), normalize=False)
        assert np.array_equal(_bits(alone), _bits(rows[cu[s]:cu[s + 1]])), (dims, ftype, s)
    m.close()


def test_token_rows_device_form_and_f16_rows(make_model):
    path, hp = make_model("minilm-l6", "f16", 6)
    m = pybert.BertModel(path)
    sents, toks, cu = _batch(hp)
    rows, emb = m.eval_packed_tokens(toks, cu, normalize=True, with_embeddings=True)
    hip = _Hip()
    T, B, H = int(cu[-1]), len(sents), hp.n_embd
    d_tok, d_cu = hip.upload(toks), hip.upload(cu)
    d_rows, d_emb = hip.upload(np.full((T, H), np.nan, np.float16)), hip.upload(np.full((B, H), np.nan, np.float32))
    m.reserve(T, B)
    m.eval_packed_tokens_device(d_tok, d_cu, B, T, 64, d_rows, d_emb, normalize=True, f16=True)
    got_emb = hip.download(d_emb, (B, H))
    got = np.empty((T, H), dtype=np.float16)
    assert hip.lib.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(d_rows), C.c_size_t(got.nbytes), 2) == 0
    assert np.array_equal(_bits(got_emb), _bits(emb)) and np.array_equal(_bits(got), _bits(rows.astype(np.float16)))
    # max_len broken by the last sentence: NaN rows for its tokens only, a NaN embedding, the status word
    m.eval_packed_tokens_device(d_tok, d_cu, B, T, 48, d_rows, None, normalize=True, f16=True)
    assert hip.lib.hipDeviceSynchronize() == 0
    assert hip.lib.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(d_rows), C.c_size_t(got.nbytes), 2) == 0
    assert np.isnan(got[cu[-2]:]).all() and np.array_equal(_bits(got[:cu[-2]]), _bits(rows[:cu[-2]].astype(np.float16))) and m.check() == 1
    hip.free(d_tok, d_cu, d_rows, d_emb)
    m.close()


def test_a_one_launch_batch_takes_the_layered_route_for_token_rows(make_model):
    path, hp = make_model("minilm-l6", "f16", 6)
    m = pybert.BertModel(path)
    m.set_option("latency", "0")
    toks = gf.synthetic_token_ids(3, 128, hp.n_vocab, seed=11).astype(np.int32).reshape(-1)
    cu = _cu([128] * 3)
    m.profile(True)
    plain = m.eval_packed(toks, cu)
    assert "model_kernel" in m.profile_report()
    rows, emb = m.eval_packed_tokens(toks, cu, normalize=True, with_embeddings=True)
    rep = m.profile_report()
    assert "token_rows" in rep and rep["token_rows"]["launches"] == 1 and "model_kernel" not in rep, sorted(rep)
    assert np.array_equal(_bits(emb), _bits(plain)) and np.isfinite(rows).all()
    assert np.array_equal(_bits(m.eval_packed(toks, cu)), _bits(plain))
    rep = m.profile_report()
    assert "model_kernel" in rep and "token_rows" not in rep, sorted(rep)
    m.close()


def test_host_form_cut_into_chunks_keeps_the_bits(make_model):
    path, hp = make_model("tiny", "f16", 2)
    m = pybert.BertModel(path)
    sents, toks, cu = _batch(hp)
    want_rows, want_emb = m.eval_packed_tokens(toks, cu, normalize=True, with_embeddings=True)
    m.set_option("chunk_tokens", "70")          # 54 | 65 | 48 | 64 tokens: cut three times
    m.profile(True)
    rows, emb = m.eval_packed_tokens(toks, cu, normalize=True, with_embeddings=True)
    assert m.profile_report()["token_rows"]["launches"] == 4
    assert np.array_equal(_bits(rows), _bits(want_rows)) and np.array_equal(_bits(emb), _bits(want_emb))
    m.close()


def test_encode_tokens_matches_tokenize_and_eval(text_model):
    m = pybert.BertModel(text_model[0])
    texts = ["hello world!", "testing tests, a b c.", "", "a " * 80]
    rows, cu = m.encode_tokens(texts, normalize=True)
    ids = [m.tokenize(t) for t in texts]
    assert np.array_equal(cu, _cu([len(i) for i in ids])) and len(ids[3]) == m.n_max_tokens
    want = m.eval_packed_tokens(np.concatenate(ids).astype(np.int32), cu, normalize=True)
    assert np.array_equal(_bits(rows), _bits(want))
    m.close()


# ------------------------------------------------------------------------------------------------
# MaxSim, op level
# ------------------------------------------------------------------------------------------------
Q_LENS = [1, 31, 32, 33, 130]
D_LENS = [1, 31, 32, 33, 127, 128, 129, 513]


@pytest.fixture(scope="module")
def ms_model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.close()


def _device_maxsim(m, q16, qcu, d16, dcu, pairs, mean, scores_before=None):
    """bert_hip_maxsim_device on f16 rows: every row of q16 / d16 is uploaded, whatever the cu arrays cover"""
    hip = _Hip()
    n_q, n_d = len(qcu) - 1, len(dcu) - 1
    shape = (n_q, n_d) if pairs is None else (len(pairs),)
    before = np.full(shape, np.nan, np.float32) if scores_before is None else scores_before
    ptrs = [hip.upload(q16), hip.upload(np.asarray(qcu, np.int32)), hip.upload(d16), hip.upload(np.asarray(dcu, np.int32)), hip.upload(before)]
    d_pairs = hip.upload(np.asarray(pairs, np.int32)) if pairs is not None else None
    m.maxsim_device(ptrs[0], ptrs[1], n_q, ptrs[2], ptrs[3], n_d, q16.shape[1], d_pairs, 0 if pairs is None else len(pairs), ptrs[4], mean)
    out = hip.download(ptrs[4], shape)
    hip.free(*(ptrs + ([d_pairs] if d_pairs else [])))
    return out


_MS_CASES = {}


def _ms_case(H):
    """the sets of one H and their float64 references, made once: NaN rows in front of, between (sentences no pair names) and behind"""
    if H not in _MS_CASES:
        rng = np.random.default_rng(1000 + H)
        q, qcu, qreal = mr.packed_set(rng, Q_LENS, H, front=2, behind=3, junk_every=2)
        d, dcu, dreal = mr.packed_set(rng, D_LENS, H, front=1, behind=5, junk_every=3)
        pairs = np.array([(a, b) for a in qreal for b in dreal], dtype=np.int32)
        pairs = np.concatenate([pairs[rng.permutation(len(pairs))], pairs[:7]])          # arbitrary order, with repeats
        q16, d16 = q.astype(np.float16), d.astype(np.float16)
        ref = {mean: mr.maxsim_reference(np.nan_to_num(q16.astype(np.float64)), qcu, np.nan_to_num(d16.astype(np.float64)), dcu, pairs, mean) for mean in (False, True)}
        _MS_CASES[H] = (q, qcu, qreal, d, dcu, dreal, pairs, q16, d16, ref)
    return _MS_CASES[H]


@pytest.mark.parametrize("H", [8, 24, 64, 384, 768, 1024])
def test_maxsim_against_the_reference(ms_model, H):
    q, qcu, qreal, d, dcu, dreal, pairs, q16, d16, ref = _ms_case(H)
    for mean in (False, True):
        want, bound = ref[mean]
        # list form, host entry (uploads rows cu[0] .. cu[n]: NaN rows in front and between) and device entry (NaN rows behind as well)
        host = ms_model.maxsim(q, qcu, d, dcu, pairs, mean)
        dev = _device_maxsim(ms_model, q16, qcu, d16, dcu, pairs, mean)
        _hold(host, want, bound, f"maxsim H {H} mean {int(mean)}")
        assert np.array_equal(_bits(host), _bits(dev))
        # all pairs over the real sentences alone (no sentence of NaN rows), NaN rows in front and behind: the list form's bits
        rq = np.concatenate([q16[qcu[a]:qcu[a + 1]] for a in qreal]); rd = np.concatenate([d16[dcu[b]:dcu[b + 1]] for b in dreal])
        nanq, nand = np.full((3, H), np.nan, np.float16), np.full((2, H), np.nan, np.float16)
        allp = _device_maxsim(ms_model, np.concatenate([nanq, rq, nanq]), _cu(Q_LENS) + 3, np.concatenate([nand, rd, nand]), _cu(D_LENS) + 2, None, mean)
        assert allp.shape == (len(Q_LENS), len(D_LENS)) and np.isfinite(allp).all()
        lookup = {(a, b): host[i] for i, (a, b) in enumerate(pairs.tolist())}
        for i, a in enumerate(qreal):
            for j, b in enumerate(dreal):
                assert _bits(np.float32(allp[i, j])) == _bits(np.float32(lookup[(a, b)])), (H, mean, i, j)
        # a pair alone and at another position: the same bits
        a, b = qreal[4], dreal[7]
        alone = ms_model.maxsim(q[qcu[a]:qcu[a + 1]], [0, Q_LENS[4]], d[dcu[b]:dcu[b + 1]], [0, D_LENS[7]], None, mean)
        assert _bits(np.float32(alone[0, 0])) == _bits(np.float32(lookup[(a, b)]))
        # repeats agree with each other
        assert np.array_equal(_bits(host[-7:]), _bits(np.array([lookup[tuple(p)] for p in pairs[-7:].tolist()], np.float32)))


@pytest.mark.parametrize("H", [8, 24, 384, 1024])
def test_maxsim_all_negative_similarities(ms_model, H):
    """documents near -Q: a padded document slot that entered the max as 0 would lift a score to 0 or above; a padded query slot that
    entered the sum would show in the queries of 1 and 33 tokens"""
    rng = np.random.default_rng(2000 + H)
    q, qcu, d, dcu = mr.negative_sets(rng, [1, 33, 31, 64], [1, 31, 33, 129], H)
    for mean in (False, True):
        want, bound = mr.maxsim_reference(mr.round_f16(q), qcu, mr.round_f16(d), dcu, None, mean)
        got = ms_model.maxsim(q, qcu, d, dcu, None, mean)
        assert (got < 0).all() and (want < -0.5).all(), (H, got)
        _hold(got, want, bound, f"maxsim negative H {H} mean {int(mean)}")


def test_maxsim_error_cases(ms_model):
    H = 24
    rng = np.random.default_rng(7)
    q, qcu, _ = mr.packed_set(rng, [3, 40, 5], H)
    d, dcu, _ = mr.packed_set(rng, [33, 2, 64, 7], H)
    good = ms_model.maxsim(q, qcu, d, dcu)
    # the host form refuses, outputs untouched
    out = np.full((3, 4), 5.0, np.float32)
    bad_qcu = qcu.copy(); bad_qcu[2] = bad_qcu[1]                           # an empty sentence
    desc_dcu = dcu.copy(); desc_dcu[2] = desc_dcu[1] - 1                    # a descending entry
    for args in ((q, bad_qcu, d, dcu, None), (q, qcu, d, desc_dcu, None), (q, qcu, d, dcu, [(0, 4)]), (q, qcu, d, dcu, [(-1, 0)]), (q, qcu, d, dcu, [(3, 0)])):
        o = out if args[4] is None else np.full(1, 5.0, np.float32)
        with pytest.raises(ValueError):
            ms_model.maxsim(*args, out=o)
        assert (o == 5.0).all()
    for badH in (4, 12, 1032):
        with pytest.raises(ValueError):
            ms_model.maxsim(np.zeros((2, badH), np.float32), [0, 2], np.zeros((2, badH), np.float32), [0, 2])
    # the device form: NaN for exactly the bad pairs, the neighbours' bits as they were
    q16, d16 = q.astype(np.float16), d.astype(np.float16)
    got = _device_maxsim(ms_model, q16, bad_qcu, d16, desc_dcu, None, False)
    bad = np.zeros((3, 4), bool); bad[1, :] = True; bad[:, 1] = True       # query 1 is empty, document 1 descends
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    # (query 2 and document 2 now start early: query 0 against documents 0 and 3 are the pairs whose ranges did not change)
    assert np.array_equal(_bits(got[0, [0, 3]]), _bits(good[0, [0, 3]]))
    pairs = np.array([(0, 0), (3, 0), (0, -1), (2, 3), (0, 4), (-5, 9), (2, 3)], np.int32)
    got = _device_maxsim(ms_model, q16, qcu, d16, dcu, pairs, False)
    assert np.isnan(got[[1, 2, 4, 5]]).all()
    assert np.array_equal(_bits(got[[0, 3, 6]]), _bits(np.array([good[0, 0], good[2, 3], good[2, 3]], np.float32)))


# ------------------------------------------------------------------------------------------------
# MaxSim in several launches: one workgroup per pair, at most 2^23 pairs (2^31 threads) per launch; the tuning key
# "maxsim_launch_pairs" lowers that, so the launch edges are reached at small shapes.  A pair's bits depend on its own rows alone:
# every result under the key at 7 equals the one at 0 bit for bit.
# ------------------------------------------------------------------------------------------------
LAUNCH_PAIRS = 7
PREFILL = 0x7FC12345                     # a NaN no kernel writes (maxsim's own NaN is 0x7FC00000)


def _launch_sets(H=24):
    rng = np.random.default_rng(31)
    q, qcu, _ = mr.packed_set(rng, [1, 31, 33, 32, 130], H)
    d, dcu, _ = mr.packed_set(rng, [33, 1, 129], H)
    return q, qcu, d, dcu


def _with_key(m, value, fn):
    m.set_option("maxsim_launch_pairs", str(value))
    try:
        return fn()
    finally:
        m.set_option("maxsim_launch_pairs", "0")


def _device_maxsim_prefilled(m, q16, qcu, d16, dcu, pairs, n_out, extra, mean=False, stream=0, hip=None):
    """bert_hip_maxsim_device into a buffer of n_out + extra words, all PREFILL before: (the n_out scores, the bits of the words behind)"""
    from hip_graph import Hip
    hip = hip or Hip()
    n_q, n_d = len(qcu) - 1, len(dcu) - 1
    ptrs = [hip.upload(q16), hip.upload(np.asarray(qcu, np.int32)), hip.upload(d16), hip.upload(np.asarray(dcu, np.int32)),
            hip.upload(np.full(n_out + extra, PREFILL, np.uint32))]
    d_pairs = hip.upload(np.asarray(pairs, np.int32)) if pairs is not None else None
    m.maxsim_device(ptrs[0], ptrs[1], n_q, ptrs[2], ptrs[3], n_d, q16.shape[1], d_pairs, 0 if pairs is None else len(pairs), ptrs[4], mean, stream)
    out = hip.download(ptrs[4], (n_out + extra,), np.uint32)
    hip.free(*(ptrs + ([d_pairs] if d_pairs else [])))
    return out[:n_out].view(np.float32), out[n_out:]


def test_maxsim_in_several_launches_all_pairs_and_mean(ms_model):
    """5 x 3 sets: launches of 7 pairs begin inside rows 2 and 4 of the score matrix"""
    q, qcu, d, dcu = _launch_sets()
    q16, d16 = q.astype(np.float16), d.astype(np.float16)
    for mean in (False, True):
        whole = ms_model.maxsim(q, qcu, d, dcu, None, mean)
        want, bound = mr.maxsim_reference(mr.round_f16(q), qcu, mr.round_f16(d), dcu, None, mean)
        assert whole.shape == (5, 3) and (np.abs(whole - want) <= bound).all()
        for key in (LAUNCH_PAIRS, 1, 15, 16):
            cut = _with_key(ms_model, key, lambda: ms_model.maxsim(q, qcu, d, dcu, None, mean))
            assert np.array_equal(_bits(cut), _bits(whole)), (mean, key)
        dev, behind = _with_key(ms_model, LAUNCH_PAIRS, lambda: _device_maxsim_prefilled(ms_model, q16, qcu, d16, dcu, None, 15, 9, mean))
        assert np.array_equal(_bits(dev.reshape(5, 3)), _bits(whole)) and (behind == PREFILL).all(), mean
    # a value above the bound is the bound, a value below 1 the default
    for key in (2 ** 23 + 1, 2 ** 31 - 1, -3):
        cut = _with_key(ms_model, key, lambda: ms_model.maxsim(q, qcu, d, dcu))
        assert np.array_equal(_bits(cut), _bits(ms_model.maxsim(q, qcu, d, dcu))), key


def test_maxsim_in_several_launches_pair_list_with_nan_cases_at_the_edges(ms_model):
    """20 pairs in launches of 7: an index out of range and an empty sentence on both sides of the edges at 7 and 14; nothing behind
    the list is written"""
    q, qcu, d, dcu = _launch_sets()
    q16, d16 = q.astype(np.float16), d.astype(np.float16)
    empty_qcu = qcu.copy()
    empty_qcu[3] = empty_qcu[4]                                          # query 3 is empty; query 2 takes its rows, 0, 1 and 4 are as they were
    pairs = np.array([(0, 0), (1, 2), (2, 1), (4, 0), (0, 2), (1, 1), (0, 3),          # 6: document out of range
                      (3, 0), (2, 2), (4, 1), (0, 1), (1, 0), (2, 0), (3, 2),          # 7, 13: the empty query
                      (5, 1), (4, 2), (0, 0), (-1, 0), (2, 1), (1, 2)], np.int32)      # 14, 17: query out of range
    nan_at = [6, 7, 13, 14, 17]
    whole, behind0 = _device_maxsim_prefilled(ms_model, q16, empty_qcu, d16, dcu, pairs, 20, 12)
    cut, behind = _with_key(ms_model, LAUNCH_PAIRS, lambda: _device_maxsim_prefilled(ms_model, q16, empty_qcu, d16, dcu, pairs, 20, 12))
    assert np.array_equal(_bits(cut), _bits(whole)) and (behind == PREFILL).all() and (behind0 == PREFILL).all()
    assert np.isnan(cut[nan_at]).all() and (_bits(cut[nan_at]) != PREFILL).all() and np.isfinite(np.delete(cut, nan_at)).all()
    good = ms_model.maxsim(q, qcu, d, dcu)
    keep = [i for i in range(20) if i not in nan_at and pairs[i, 0] != 2]
    assert np.array_equal(_bits(cut[keep]), _bits(np.array([good[a, b] for a, b in pairs[keep].tolist()], np.float32)))


def test_token_index_rescore_with_maxsim_in_several_launches(ms_model):
    import token_index_reference as tref

    dim = 24
    rng = np.random.default_rng(32)
    d, dcu = tref.documents(rng, 60, dim)
    q, qcu = tref.queries(rng, dim, [1, 33, 31, 64, 128])
    ix = ms_model.token_index(dim)
    assert ix.add(d, dcu) == 0
    cand = rng.integers(-1, 60, (5, 33)).astype(np.int32)               # 165 pairs: 24 launches of 7 (the last of 4)
    whole = ix.rescore(q, qcu, cand, 10)
    cut = _with_key(ms_model, LAUNCH_PAIRS, lambda: ix.rescore(q, qcu, cand, 10))
    assert np.array_equal(cut[0], whole[0]) and np.array_equal(_bits(cut[1]), _bits(whole[1]))
    assert tref.same_result(whole, tref.rescore_expected(ms_model.maxsim(q, qcu, d, dcu), cand, 10))
    ix.close()


def test_maxsim_in_several_launches_is_captured_and_replayed(ms_model):
    """a captured bert_hip_maxsim_device call holds one kernel node per launch and replays to the eager bits"""
    from hip_graph import Hip
    hip = Hip()
    q, qcu, d, dcu = _launch_sets()
    eager = ms_model.maxsim(q, qcu, d, dcu)
    ptrs = [hip.upload(q.astype(np.float16)), hip.upload(qcu.astype(np.int32)), hip.upload(d.astype(np.float16)), hip.upload(dcu.astype(np.int32)),
            hip.nans((5, 3), np.float32)]
    s = hip.stream()
    for key, nodes in ((LAUNCH_PAIRS, 3), (0, 1)):
        def body():
            with hip.capture(s) as cap:
                ms_model.maxsim_device(ptrs[0], ptrs[1], 5, ptrs[2], ptrs[3], 3, q.shape[1], None, 0, ptrs[4], False, s)
            return cap
        cap = _with_key(ms_model, key, body)
        assert cap.status == 0 and cap.graph and hip.kernel_nodes(cap.graph) == nodes, key
        ex = hip.instantiate(cap.graph)
        for _ in range(2):
            hip.poison(ptrs[4], (5, 3), np.float32)
            hip.launch(ex, s)
            assert np.array_equal(_bits(hip.download(ptrs[4], (5, 3), np.float32)), _bits(eager)), key
        hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(*ptrs)


def test_maxsim_of_more_than_two_to_the_24_pairs(ms_model):
    """4097 x 4096 one-token sets at H = 8, all pairs: 16 781 312 workgroups, which as one launch of 256 threads each would pass 2^32
    threads.  The rows hold small integers, so q @ d.T in float32 is the exact expected matrix; the output starts as NaN and every
    element must be equal.  (Wall time of the call and its synchronisation: profiles/launch_geometry_tests.txt.)"""
    import time
    from hip_graph import Hip
    hip = Hip()
    n_q, n_d, H = 4097, 4096, 8
    assert n_q * n_d == 16781312 > 2 ** 24
    rng = np.random.default_rng(33)
    q = rng.integers(-4, 5, (n_q, H)).astype(np.float32)
    d = rng.integers(-4, 5, (n_d, H)).astype(np.float32)
    want = q @ d.T
    assert want.dtype == np.float32 and np.array_equal(want.astype(np.float64), q.astype(np.float64) @ d.astype(np.float64).T)
    ptrs = [hip.upload(q.astype(np.float16)), hip.upload(np.arange(n_q + 1, dtype=np.int32)), hip.upload(d.astype(np.float16)),
            hip.upload(np.arange(n_d + 1, dtype=np.int32)), hip.nans((n_q, n_d), np.float32)]
    hip.sync()
    t0 = time.perf_counter()
    ms_model.maxsim_device(ptrs[0], ptrs[1], n_q, ptrs[2], ptrs[3], n_d, H, None, 0, ptrs[4])
    hip.sync()
    print(f"maxsim of {n_q} x {n_d} one-token sets at H = {H}: {1e3 * (time.perf_counter() - t0):.1f} ms")
    got = hip.download(ptrs[4], (n_q, n_d), np.float32)
    hip.free(*ptrs)
    wrong = np.flatnonzero(~(got == want).ravel())
    assert wrong.size == 0, (wrong.size, "first at pair", int(wrong[0]), "unwritten", int(np.isnan(got).sum()))


# ------------------------------------------------------------------------------------------------
# the example program
# ------------------------------------------------------------------------------------------------
def test_bert_search_maxsim(text_model, tmp_path):
    path, _ = text_model
    lines = ["hello world", "testing servers, clients!", "embedding test.", "pool index search row", "long text window", "a b c d e f g h i j a b c",
             "hello hello world world", "search row index", "text window stride long text"]
    query = "long text window stride"
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    run = lambda flags: subprocess.run([exe, "-m", path, "-f", str(f), "-k", "2"] + flags, input=query + "\nq\n", capture_output=True, text=True, timeout=300)
    m = pybert.BertModel(path)
    ix = m.index()
    assert ix.add_texts(lines) == 0
    ids, scores = ix.search_texts([query], k=5)
    # without the flag: today's output, byte for byte
    r = run([])
    assert r.returncode == 0, r.stderr
    prompt = "Enter a text to find similar texts (enter 'q' to quit): "
    want = f"Loading texts from {f}...\nLoaded {len(lines)} lines.\n{prompt}\nClosest texts:\n"
    want += "".join(f"{i + 1}. {lines[ids[0][i]]}\n (similarity score: {scores[0][i]:.4f})\n" for i in range(2)) + prompt + "\n"
    assert r.stdout == want
    # with it: the candidates' order by pybert's encode_tokens + maxsim
    cands = [lines[i] for i in ids[0]]
    rows, cu = m.encode_tokens([query] + cands, normalize=True)
    ms = m.maxsim(rows[:cu[1]], [0, cu[1]], rows[cu[1]:], cu[1:] - cu[1], [(0, j) for j in range(5)])
    order = sorted(range(5), key=lambda j: -ms[j])
    r = run(["--maxsim", "5"])
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    shown = [l[3:] for l in out if l[:3] in ("1. ", "2. ")]
    assert shown == [cands[order[0]], cands[order[1]]]
    assert [l for l in out if "MaxSim score" in l] == [f" (MaxSim score: {ms[order[i]]:.4f})" for i in range(2)]
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert "--maxsim N" in r.stderr
    r = run(["--maxsim", "1"])
    assert r.returncode == 2 and "--maxsim" in r.stderr
    ix.close(); m.close()


def test_worst_fractions_are_recorded():
    """(last in the file) every bound above was met with room: the figures, for the log"""
    for what, frac in sorted(_WORST.items()):
        print(f"{what}: {frac:.3f}")
    assert all(f <= 1.0 for f in _WORST.values())
