"""GPU tests of the learned sparse embeddings (bert_hip.h "learned sparse embeddings"): the vocabulary kernel (matrix-core and plain
forms) and the top-k launch at op level against float64 and the NumPy rule, bit stability, the whole path end to end against a float64
model, the text level, errors and stream capture."""
import dataclasses
import os

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import hip_graph
import sparse_reference as sr

pytestmark = pytest.mark.gpu


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------
# 1. the vocabulary kernel at op level
# ------------------------------------------------------------------------------------------------
LENS = {"one": [1], "mixed": [1, 4, 5, 128], "sub-block": [31, 32, 33], "tile-edge": [128, 128], "beside-edge": [127, 1, 128], "five-tiles": [513],
        "forty": [1 + i % 3 for i in range(40)]}
FORMS = [("mfma", 8), ("mfma", 24), ("mfma", 64), ("mfma", 384), ("mfma", 768), ("mfma", 1024), ("plain", 26), ("plain", 384)]
VOCABS = [1, 31, 33, 250, 1000]
_INPUTS = {}


def _op_inputs(H, V, T):
    """t [T, H], E [V, H] as f32 values that f16 holds exactly, bias [V].  Feature 0 of every token is >= 1, so that a vocabulary row of
    (-5, 0, ...) has only negative products; column 0 is that row (z < 0) and, where there is one, column 1 a zero row with bias 0 (z = 0).
    Shared among the cases, read-only."""
    key = (H, V, T)
    if key not in _INPUTS:
        rng = np.random.default_rng(7 * H + 3 * V + T)
        t = rng.normal(0, 1, (T, H)).astype(np.float16)
        t[:, 0] = np.abs(t[:, 0]) + np.float16(1)
        E = rng.normal(0, 1, (V, H)).astype(np.float16)
        bias = rng.normal(-0.5 * np.sqrt(H), np.sqrt(H), V).astype(np.float32)
        E[0] = 0; E[0, 0] = -5; bias[0] = 0
        if V > 1:
            E[1] = 0; bias[1] = 0
        for a in (t, E, bias):
            a.setflags(write=False)
        _INPUTS[key] = (t, E, bias)
    return _INPUTS[key]


@pytest.mark.parametrize("lens_name", list(LENS))
@pytest.mark.parametrize("form,H", FORMS)
def test_vocabulary_kernel_matches_float64(form, H, lens_name):
    """Both forms against float64 within sparse_bound (drows = 0) for every V; NaN rows around the operands and garbage in the output (the
    hook's), so the launch reads nothing outside and zero-fills itself; columns whose z is negative or zero give exactly +0."""
    lens = LENS[lens_name]
    T = sum(lens)
    for V in VOCABS:
        t, E, bias = _op_inputs(H, V, T)
        want = sr.sparse(t, E, bias, lens)
        for dtype in ((np.float16,) if form == "mfma" else (np.float16, np.float32)):
            got = pybert.test_sparse_vocab(t.astype(dtype), E.astype(dtype), bias, _cu(lens), form)
            assert got is not None and got.shape == (len(lens), V), (form, H, V)
            assert np.isfinite(got).all() and not np.signbit(got).any(), (form, H, V, lens_name)
            bound = sr.sparse_bound(t, 0.0, E, bias, lens, mfma=form == "mfma")
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), (form, H, V, lens_name, float((err / bound).max()))
            assert (_bits(got[:, :2]) == 0).all(), (form, H, V, lens_name)
            assert ((got == 0) == (want == 0)).mean() > 0.99
            if V >= 250 and max(lens) <= 33:
                assert 0.05 < (got == 0).mean() < 0.95             # (short sentences: both sides of the relu edge are there)


def test_vocabulary_kernel_refusals():
    t, E, bias = _op_inputs(24, 33, 5)
    cu = _cu([5])
    assert pybert.test_sparse_vocab(t[:, :20], E[:, :20], bias, cu, "mfma") is None           # H = 20: not a multiple of 8
    assert pybert.test_sparse_vocab(t.astype(np.float32), E, bias, cu, "mfma") is None
    assert pybert.test_sparse_vocab(t[:, :20], E[:, :20], bias, cu, "plain") is not None


@pytest.mark.parametrize("form,H", [("mfma", 64), ("mfma", 384), ("mfma", 768), ("plain", 26)])
def test_a_sentence_keeps_its_bits(form, H):
    """A sentence's row has the same bits alone, behind sentences of 5 and 37 tokens, across a tile edge (behind 120 tokens: slots 120 ..
    159 of 128- and 64-slot tiles), in other batch sizes, served as a chunk of its own, and from run to run."""
    V = 250
    t, E, bias = _op_inputs(H, V, 513)
    sent = t[100:140]
    alone = pybert.test_sparse_vocab(sent, E, bias, _cu([40]), form)
    assert _same(alone, pybert.test_sparse_vocab(sent, E, bias, _cu([40]), form))
    for front in ([5, 37], [120], [64, 56, 3], [1] * 30 + [128]):
        n = sum(front)
        rows = np.concatenate([t[200:200 + n], sent, t[400:407]])
        lens = front + [40, 7]
        got = pybert.test_sparse_vocab(rows, E, bias, _cu(lens), form)
        assert _same(got[len(front)], alone[0]), (form, H, front)
        part = pybert.test_sparse_vocab(rows, E, bias, _cu(lens), form, s0=len(front), ns=1)
        assert _same(part, alone), (form, H, front)
        assert _same(pybert.test_sparse_vocab(rows, E, bias, _cu(lens), form, s0=1, ns=len(front)), got[1:len(front) + 1])


# ------------------------------------------------------------------------------------------------
# 2. top-k at op level
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 300, 30522])
@pytest.mark.parametrize("k", [1, 10, 256])
def test_topk_launch_follows_the_rule(V, k):
    """Rows with more than k, fewer than k and no positive weights, exact ties (also across the k-th place), negative and NaN entries:
    ids and weights bit-equal to the NumPy rule."""
    rng = np.random.default_rng(V + k)
    w = np.zeros((7, V), dtype=np.float32)
    w[0] = rng.gamma(1.0, 1.0, V)                              # all positive
    w[1, rng.permutation(V)[:min(V, 7)]] = rng.gamma(1.0, 1.0, min(V, 7))        # few positives
    w[3] = np.round(rng.gamma(1.0, 1.0, V) * 4) / 4            # many exact ties, zeros among them
    w[4] = 0.75                                                # one value everywhere
    w[5] = rng.normal(0, 1, V)                                 # negatives do not count
    w[5, ::3] = np.nan
    w[6] = w[0]
    w[6, rng.permutation(V)[:V // 2]] = 0
    got = pybert.test_sparse_topk(w, k)
    assert got is not None
    ids, wt = got
    want_ids, want_w = sr.topk(w, k)
    assert np.array_equal(ids, want_ids), (V, k, np.argwhere(ids != want_ids)[:4])
    assert _same(wt, want_w)
    assert (ids[2] == -1).all() and (_bits(wt[2]) == 0).all()


def test_topk_launch_refusals():
    w = np.ones((2, 40), dtype=np.float32)
    assert pybert.test_sparse_topk(w, 257) is None and pybert.test_sparse_topk(w, 256) is not None


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
DIMS, e2e_batches = sr.DIMS, sr.e2e_batches
_FILES = {}


def _model_file(model_dir, dims, ftype, mlm_head=True, n_labels=0):
    key = (dims, ftype, mlm_head, n_labels)
    if key not in _FILES:
        path = os.path.join(model_dir, f"sparse_{dims}_{ftype}_{int(mlm_head)}_{n_labels}.bin")
        gf.write_model(path, DIMS[dims], gf.synthetic_weights(DIMS[dims], sr.E2E_SEED, n_labels=n_labels, mlm_head=mlm_head), gf.FTYPE_BY_NAME[ftype])
        _FILES[key] = path
    return _FILES[key]


# ------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------
# drows: twice what the PARENT commit — which has no MLM head, but the same encoder — leaves between bert_hip_eval_packed_tokens'
# un-normalised rows and the float64 states on the very batches below, as a fraction of the token's largest state
# (profiles/sparse_parity.txt, written by tools/sparse_parity.py against the parent's library).
PARENT_STATE_ERROR = {("tiny", "f32"): 2.159e-06, ("tiny", "f16"): 2.264e-03, ("tiny", "q4_0"): 2.923e-03, ("tiny-d64", "f16"): 2.569e-03,
                      ("minilm-l6", "f16"): 1.366e-03}
assert list(PARENT_STATE_ERROR) == sr.E2E_MODELS


@pytest.mark.parametrize("dims,ftype", list(PARENT_STATE_ERROR))
def test_sparse_weights_match_float64(model_dir, dims, ftype):
    """The dense rows end to end within sparse_bound of the float64 model, the states allowed twice the parent's own error and the transform
    its derived bound; top-k is the rule applied to the dense rows; the launches appear under their names."""
    drel = 2 * PARENT_STATE_ERROR[(dims, ftype)]
    path = _model_file(model_dir, dims, ftype)
    ref = sr.Model(path)
    m = pybert.BertModel(path)
    assert m.has_mlm_head
    f32_route = ftype == "f32"
    Wt, bt, g, b, E, bias = ref.mlm_weights()
    for name, (toks, cu, sents) in e2e_batches(dims).items():
        m.profile(True)
        got = m.sparse_packed(toks, cu)
        names = set(m.profile_report())
        m.profile(False)
        assert {"mlm_transform", "mlm_layernorm", "sparse_vocab"} <= names and ("sparse_finish" in names) == (not f32_route), names
        assert got.shape == (len(sents), ref.hp.n_vocab) and np.isfinite(got).all() and not np.signbit(got).any()
        worst = 0.0
        for row, s in zip(got, sents):
            x = ref.states(s)
            dx = drel * np.abs(x).max(axis=1, keepdims=True)
            t = ref.transform(x)
            dt = sr.transform_bound(x, dx, Wt, bt, g, b, f32_route, w_rounded=ftype not in ("f16", "f32"))
            want = sr.sparse(t, E, bias, [len(s)])[0]
            bound = sr.sparse_bound(t, dt, E, bias, [len(s)], mfma=not f32_route, e_rounded=ftype != "f16")[0]
            err = np.abs(row.astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (dims, ftype, name, len(s), float((err / bound).max()), float(err.max()))
        zero = float((got == 0).mean())
        print(f"{dims} {ftype} {name}: worst error / bound = {worst:.3e}; {zero:.3f} of the weights are zero")
        assert 0.15 <= zero <= 0.85
        for k in (10, 256):
            ids, wt = m.sparse_packed(toks, cu, k)
            want_ids, want_w = sr.topk(got, k)
            assert np.array_equal(ids, want_ids) and _same(wt, want_w), (dims, ftype, name, k)
    m.close()


def test_topk_runs_in_chunks_of_sentences(model_dir):
    """300 sentences at V = 30 522 are more than the 32 MiB scratch holds (274): the top-k form runs in two chunks and still gives the
    rule applied to the dense form's rows, before and after bert_hip_reserve."""
    m = pybert.BertModel(_model_file(model_dir, "minilm-l6", "f16"))
    rng = np.random.default_rng(9)
    lens = [1 + i % 3 for i in range(300)]
    toks, cu, _ = sr.batch(rng, DIMS["minilm-l6"], lens)
    dense = m.sparse_packed(toks, cu)
    for reserve in (False, True):
        if reserve:
            m.reserve(int(cu[-1]), len(lens))
        ids, wt = m.sparse_packed(toks, cu, 10)
        want_ids, want_w = sr.topk(dense, 10)
        assert np.array_equal(ids, want_ids) and _same(wt, want_w)
    # a sentence alone: the bits it has in the batch
    for b in (0, 5, 273, 274, 299):
        assert _same(m.sparse_packed(toks[cu[b]:cu[b + 1]], _cu([lens[b]]))[0], dense[b])
    m.close()


# ------------------------------------------------------------------------------------------------
# 4. composition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ftype", [("tiny", "f16"), ("tiny", "f32"), ("minilm-l6", "f16")])
def test_existing_entry_points_keep_their_bits(model_dir, dims, ftype):
    """The same encoder with and without the MLM head: eval_packed under every pooling setting and the token rows with their embeddings
    return equal bits, also after a sparse call on the head-carrying context; with both heads, the scores are the classification-only
    model's."""
    plain, both = pybert.BertModel(_model_file(model_dir, dims, ftype, False, 2)), pybert.BertModel(_model_file(model_dir, dims, ftype, True, 2))
    assert not plain.has_mlm_head and both.has_mlm_head and plain.n_labels == both.n_labels == 2
    toks, cu, _ = e2e_batches(dims)["long"]
    both.sparse_packed(toks, cu, 5)
    for pooling in ("mean", "cls"):
        for normalize in ("1", "0"):
            for m in (plain, both):
                m.set_option("pooling", pooling); m.set_option("normalize", normalize)
            want = plain.eval_packed(toks, cu)
            assert np.isfinite(want).all() and _same(both.eval_packed(toks, cu), want), (pooling, normalize)
    rows, emb = plain.eval_packed_tokens(toks, cu, normalize=False, with_embeddings=True)
    rows2, emb2 = both.eval_packed_tokens(toks, cu, normalize=False, with_embeddings=True)
    assert _same(rows, rows2) and _same(emb, emb2)
    assert _same(plain.score_packed(toks, cu, None), both.score_packed(toks, cu, None))
    plain.close(); both.close()


@pytest.fixture(scope="module")
def text_model(model_dir, tok_golden):
    """tiny dims over the golden tokenizer's vocabulary, with the MLM head"""
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    path = os.path.join(model_dir, "sparse_text.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=True), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return path, words


def test_text_level_is_the_packed_level(text_model):
    path, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=20)] + [""]
    ids = m.tokenize_batch(texts)
    toks, cu = np.concatenate(ids).astype(np.int32), _cu([len(i) for i in ids])
    dense = m.encode_sparse(texts)
    assert dense.shape == (21, m.n_vocab) and _same(dense, m.sparse_packed(toks, cu))
    for k in (1, 10, 256):
        got_ids, got_w = m.encode_sparse(texts, k)
        want_ids, want_w = m.sparse_packed(toks, cu, k)
        assert np.array_equal(got_ids, want_ids) and _same(got_w, want_w)
        rule_ids, rule_w = sr.topk(dense, k)
        assert np.array_equal(got_ids, rule_ids) and _same(got_w, rule_w)
    assert 0.1 < (dense == 0).mean() < 0.9
    m.close()


# ------------------------------------------------------------------------------------------------
# 5. errors
# ------------------------------------------------------------------------------------------------
def test_errors(model_dir, capfd):
    hp = DIMS["tiny"]
    toks, cu, _ = sr.batch(np.random.default_rng(0), hp, [5, 9])
    lib = pybert.lib()
    plain, with_head = pybert.BertModel(_model_file(model_dir, "tiny", "f16", False)), pybert.BertModel(_model_file(model_dir, "tiny", "f16"))
    dense = np.full((2, hp.n_vocab), 7.0, dtype=np.float32)
    ids, wt = np.full((2, 4), 7, dtype=np.int32), np.full((2, 4), 7.0, dtype=np.float32)
    i32p, f32p = pybert._i32p, pybert._f32p
    untouched = lambda: (dense == 7.0).all() and (ids == 7).all() and (wt == 7.0).all()
    capfd.readouterr()
    assert lib.bert_hip_has_mlm_head(plain.ctx) == 0 and lib.bert_hip_has_mlm_head(with_head.ctx) == 1
    # no head
    assert lib.bert_hip_sparse_packed(plain.ctx, i32p(toks), i32p(cu), 2, f32p(dense)) == -2
    assert "no MLM head" in capfd.readouterr().err
    assert lib.bert_hip_sparse_topk_packed(plain.ctx, i32p(toks), i32p(cu), 2, 4, i32p(ids), f32p(wt)) == -2
    assert "no MLM head" in capfd.readouterr().err
    assert lib.bert_hip_sparse_packed_device(plain.ctx, None, None, 2, 14, 9, None, None) == -2
    assert lib.bert_hip_sparse_topk_packed_device(plain.ctx, None, None, 2, 14, 9, 4, None, None, None) == -2
    texts = (pybert.C.c_char_p * 2)(b"a", b"b")
    assert lib.bert_hip_encode_sparse_batch(plain.ctx, 1, 2, texts, 4, i32p(ids), f32p(wt)) == -2
    assert capfd.readouterr().err.count("no MLM head") == 3 and untouched()
    # k out of range
    for k in (0, -1, 257):
        assert lib.bert_hip_sparse_topk_packed(with_head.ctx, i32p(toks), i32p(cu), 2, k, i32p(ids), f32p(wt)) == -2
        assert "outside 1 .. 256" in capfd.readouterr().err
        assert lib.bert_hip_sparse_topk_packed_device(with_head.ctx, None, None, 2, 14, 9, k, None, None, None) == -2
        assert lib.bert_hip_encode_sparse_batch(with_head.ctx, 1, 2, texts, k, i32p(ids), f32p(wt)) == -2
        capfd.readouterr()
    assert untouched()
    # a sentence that cannot be evaluated
    bad = toks.copy(); bad[3] = hp.n_vocab
    assert lib.bert_hip_sparse_packed(with_head.ctx, i32p(bad), i32p(cu), 2, f32p(dense)) == -2 and "out of range" in capfd.readouterr().err
    assert lib.bert_hip_sparse_topk_packed(with_head.ctx, i32p(toks), i32p(np.array([0, 5, 5], dtype=np.int32)), 2, 4, i32p(ids), f32p(wt)) == -2
    assert "empty input" in capfd.readouterr().err and untouched()
    # empty batch
    assert lib.bert_hip_sparse_packed(with_head.ctx, i32p(toks), i32p(cu), 0, f32p(dense)) == 0
    assert lib.bert_hip_sparse_topk_packed(with_head.ctx, i32p(toks), i32p(cu), 0, 4, i32p(ids), f32p(wt)) == 0
    assert lib.bert_hip_sparse_packed_device(with_head.ctx, None, None, 0, 0, 9, None, None) == 0
    assert lib.bert_hip_encode_sparse_batch(with_head.ctx, 1, 0, None, 4, None, None) == 0 and untouched()
    # and the calls work
    assert lib.bert_hip_sparse_packed(with_head.ctx, i32p(toks), i32p(cu), 2, f32p(dense)) == 0 and np.isfinite(dense).all() and (dense >= 0).all()
    assert lib.bert_hip_sparse_topk_packed(with_head.ctx, i32p(toks), i32p(cu), 2, 4, i32p(ids), f32p(wt)) == 0
    assert np.array_equal(ids, sr.topk(dense, 4)[0]) and _same(wt, sr.topk(dense, 4)[1])
    tok_only = pybert.BertModel(_model_file(model_dir, "tiny", "f16"), tokenizer_only=True)
    assert lib.bert_hip_has_mlm_head(tok_only.ctx) == 0
    assert lib.bert_hip_sparse_packed(tok_only.ctx, i32p(toks), i32p(cu), 2, f32p(dense)) == -1
    assert lib.bert_hip_sparse_topk_packed_device(tok_only.ctx, None, None, 2, 14, 9, 4, None, None, None) == -1
    assert lib.bert_hip_encode_sparse_batch(tok_only.ctx, 1, 2, texts, 4, i32p(ids), f32p(wt)) == -1
    capfd.readouterr()
    for m in (plain, with_head, tok_only):
        m.close()


# ------------------------------------------------------------------------------------------------
# 6. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,k", [("tiny", None), ("tiny", 10), ("minilm-l6", None), ("minilm-l6", 10)])
def test_device_forms_under_capture(model_dir, dims, k):
    """After bert_hip_reserve, both device forms are captured and replayed: the eager call's bits, which are the host form's; with other
    ids and other lengths (the same totals) written into the captured buffers, the replay gives what the host form gives for those."""
    hip = hip_graph.Hip()
    m = pybert.BertModel(_model_file(model_dir, dims, "f16"))
    hp = DIMS[dims]
    lens = [33, 5, 128, 1, 60]
    toks, cu, _ = sr.batch(np.random.default_rng(1), hp, lens)
    toks2, cu2, _ = sr.batch(np.random.default_rng(2), hp, [1, 128, 29, 64, 5])
    B, T, max_len, W = len(lens), int(cu[-1]), 128, (k or hp.n_vocab)
    assert int(cu2[-1]) == T
    d_t, d_cu, d_w, d_i = hip.upload(toks), hip.upload(cu), hip.nans((B, W)), hip.nans((B, W), np.int32)
    s = hip.stream()
    m.reserve(T, B)
    lib = pybert.lib()

    def call():
        if k is None:
            return lib.bert_hip_sparse_packed_device(m.ctx, d_t, d_cu, B, T, max_len, d_w, s)
        return lib.bert_hip_sparse_topk_packed_device(m.ctx, d_t, d_cu, B, T, max_len, k, d_i, d_w, s)

    def result():
        return (hip.download(d_i, (B, W), np.int32) if k else None), hip.download(d_w, (B, W))

    def host(tk, c):
        return m.sparse_packed(tk, c, k) if k else (None, m.sparse_packed(tk, c))

    def agree(got, want):
        return (k is None or np.array_equal(got[0], want[0])) and _same(got[1], want[1])

    def poison():
        hip.poison(d_w, (B, W)); hip.poison(d_i, (B, W), np.int32)

    want = host(toks, cu)
    assert call() == 0
    assert agree(result(), want) and m.check() == 0
    poison()
    with hip.capture(s) as cap:
        r = call()
    assert r == 0 and cap.status == hip_graph.HIP_SUCCESS and cap.graph
    assert np.isnan(hip.download(d_w, (B, W))).all(), "capturing must run nothing"
    assert hip.kernel_nodes(cap.graph) >= 5                    # (embedding, layers, transform, LayerNorm, vocabulary, ...)
    ex = hip.instantiate(cap.graph)
    for i in range(2):
        poison()
        hip.launch(ex, s)
        assert agree(result(), want), ("replay", i)
    want2 = host(toks2, cu2)
    hip.write(d_t, toks2); hip.write(d_cu, cu2)
    poison()
    hip.launch(ex, s)
    assert agree(result(), want2) and not _same(want2[1], want[1])
    poison()
    assert call() == 0 and agree(result(), want2) and m.check() == 0
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_w, d_i)
    m.close()
