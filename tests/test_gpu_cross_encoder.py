"""GPU tests of the cross-encoder feature (bert_hip.h "sentence pairs and scores"): the embedding kernels with token types and the
classification head at op level, typed passes and scores end to end against a float64 model, the text level, errors and stream capture."""
import dataclasses
import os

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import cross_encoder_reference as cer
import hip_graph
import lane_order

pytestmark = pytest.mark.gpu

WT = {"f32": 0, "f16": 1, "q4_0": 2, "q4_1": 3}


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _weight_bytes(w, ftype):
    if ftype == "f32":
        return w.astype(np.float32).view(np.uint8).reshape(-1), w.astype(np.float32)
    if ftype == "f16":
        h = w.astype(np.float16)
        return h.view(np.uint8).reshape(-1), h.astype(np.float32)
    q = gf.quantize_q4_0(w) if ftype == "q4_0" else gf.quantize_q4_1(w)
    return q.reshape(-1), (gf.dequantize_q4_0(q) if ftype == "q4_0" else gf.dequantize_q4_1(q))


# ------------------------------------------------------------------------------------------------
# 1. typed embedding at op level
# ------------------------------------------------------------------------------------------------
def _embed_want(word, typ, pos, toks, lens, first_len, gamma, beta):
    p = np.concatenate([np.arange(n) for n in lens])
    tt = np.concatenate([(np.arange(n) >= (n if first_len is None else first_len[b])).astype(np.int64) for b, n in enumerate(lens)])
    pre = word[toks] + typ[tt] + pos[p]
    mu = pre.mean(axis=1, keepdims=True)
    return (pre - mu) / np.sqrt(((pre - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5) * gamma + beta


def _first_lens(lens, which):
    return [{"-3": -3, "0": 0, "1": 1, "mid": n // 2, "len": n, "len+7": n + 7}[which] for n in lens]


_ALL = ["f32", "f16", "q4_0", "q4_1"]
# (the generic kernel serves any even H: 24, which the launcher would hand to the rows kernel, and 26, which it hands to the generic
# one, so that the existing hook runs the same kernel; q4 rows are whole blocks of 32; the f32 route has f32 tables only)
EMBED_CASES = [(form, H, [1, 4, 5, 128], ft) for form in ("grid", "search") for H in (64, 384, 768) for ft in _ALL] + \
              [("generic", H, [1, 4, 5, 128], ft) for H in (24, 26) for ft in ("f32", "f16")] + [("generic", 64, [1, 4, 5, 128], ft) for ft in ("q4_0", "q4_1")] + \
              [("f32", 64, [1, 4, 5, 128], "f32"), ("f32", 24, [5, 128, 1, 4], "f32")] + \
              [("lanes", H, lens, ft) for H in (256, 384) for lens in ([128], [128, 128], [1, 4, 5, 118], [60, 68, 1, 4, 5, 118]) for ft in _ALL]


@pytest.mark.parametrize("form,H,lens,ftype", EMBED_CASES)
def test_typed_embedding_kernels(form, H, lens, ftype):
    """word[id] + type[place >= first_len] + pos[p] -> LayerNorm against float64 on the dequantised tables, test_embed_layernorm_kernel's
    tolerance: every form, every table type, first_len from below 0 to past the end; first_len null and first_len = len give the
    existing hooks' bits."""
    rng = np.random.default_rng(H + len(ftype) + len(lens))
    V, P = 300, 128
    cu = _cu(lens)
    toks = rng.integers(0, V, size=int(cu[-1])).astype(np.int32)
    tabs = [rng.normal(0, 1, (n, H)).astype(np.float32) for n in (V, 2, P)]
    tabs[2] += np.linspace(-2, 2, P)[:, None].astype(np.float32)           # positions are distinguishable
    tabs[1][1] += 1.5                                                      # so are the types
    enc = [_weight_bytes(t, ftype) for t in tabs]
    gamma = rng.normal(1, 0.2, H).astype(np.float32); beta = rng.normal(0, 0.3, H).astype(np.float32)
    word, typ, pos = (e[1].reshape(-1, H).astype(np.float64) for e in enc)
    back = lane_order.to_rows if form == "lanes" else (lambda a: a)

    def run(fl):
        got = pybert.test_embed_ln_typed(WT[ftype], enc[0][0], enc[1][0], enc[2][0], H, gamma, beta, toks, cu, fl, form)
        assert got is not None, (form, H, ftype)
        return got

    if form == "f32":
        old = pybert.test_f32_embed_ln(tabs[0], tabs[1], tabs[2], gamma, beta, toks, cu, max(lens))
    else:
        old = pybert.test_embed_ln(WT[ftype], enc[0][0], enc[1][0], enc[2][0], H, gamma, beta, toks, cu, lanes=form == "lanes")
    untyped = run(None)
    assert _same(untyped, run(_first_lens(lens, "len"))) and _same(untyped, run(_first_lens(lens, "len+7")))
    if not (form == "generic" and H != 26):
        # (the existing hook's launch: the same kernel, but for the forced generic form at an H the launcher gives to the rows kernel;
        # the rows kernel's two forms do the same arithmetic per token)
        assert _same(untyped, old), (form, H, ftype)
    for which in ("-3", "0", "1", "mid", "len", "len+7"):
        fl = _first_lens(lens, which)
        got = back(run(fl)).astype(np.float64)
        want = _embed_want(word, typ, pos, toks, lens, fl, gamma, beta)
        err = np.abs(got - want)
        assert err.max() < 4e-3 + 1e-3 * np.abs(want).max(), (form, ftype, H, which, float(err.max()))
    assert not _same(untyped, run(_first_lens(lens, "0")))


# ------------------------------------------------------------------------------------------------
# 2. the head at op level
# ------------------------------------------------------------------------------------------------
def _head_inputs(H, NL, B, scale, seed):
    rng = np.random.default_rng(seed)
    rows = rng.normal(0, scale, (B, H)).astype(np.float32)
    Wp = rng.normal(0, 1 / np.sqrt(H), (H, H)).astype(np.float32)
    return rows, Wp, rng.normal(0, 0.1, H).astype(np.float32), rng.normal(0, 1 / np.sqrt(H), (NL, H)).astype(np.float32), rng.normal(0, 0.1, NL).astype(np.float32)


@pytest.mark.parametrize("form,H", [("mfma", 64), ("mfma", 384), ("mfma", 768), ("mfma", 1024), ("plain", 24), ("plain", 384)])
@pytest.mark.parametrize("NL", [1, 3, 8])
def test_head_kernels(form, H, NL):
    """Both head kernels against float64 within head_bound (drows = 0): batch sizes around the block of 32, row magnitudes from tanh's linear
    range to saturation, logits and sigmoid, NaN-poisoned padding; a row's bits alone, last in a block and first in the next."""
    for scale in (0.01, 1.0, 30.0):
        rows, Wp, bp, Wc, bc = _head_inputs(H, NL, 65, scale, H + NL)
        for wp_dtype in ((np.float16,) if form == "mfma" else (np.float16, np.float32)):
            W = Wp.astype(wp_dtype)
            mfma = form == "mfma"
            with pybert.test_pad(0x7E00, 0x7FC00000):
                ref = None
                for B in (1, 31, 32, 33, 65):
                    for flags in (0, 1):
                        got = pybert.test_cls_head(rows[:B], W, bp, Wc, bc, flags, form)
                        assert got is not None and got.shape == (B, NL) and np.isfinite(got).all()
                        want = cer.head(rows[:B], W, bp, Wc, bc, bool(flags))
                        # (the plain form reads the f32 rows and, given an f16 Wp, its exact values: no operand rounding)
                        bound = cer.head_bound(rows[:B], 0.0, W, bp, Wc, bc, mfma, bool(flags))
                        err = np.abs(got.astype(np.float64) - want)
                        assert (err <= bound).all(), (form, H, NL, scale, B, flags, float((err / bound).max()))
                        if flags == 0:
                            ref = got if B == 65 else ref
                            if B == 65:
                                for b in (1, 31, 32, 33):
                                    assert _same(pybert.test_cls_head(rows[:b], W, bp, Wc, bc, 0, form), got[:b])
                # row 31 (last of a block) alone, and as row 32 (first of the next block) and as row 0
                one = pybert.test_cls_head(rows[31:32], W, bp, Wc, bc, 0, form)
                moved = pybert.test_cls_head(np.concatenate([rows[:32], rows[31:32]]), W, bp, Wc, bc, 0, form)
                assert _same(one[0], ref[31]) and _same(moved[32], ref[31]) and _same(moved[31], ref[31])
    assert pybert.test_cls_head(rows[:2], Wp.astype(np.float32), bp, Wc, bc, 0, "mfma") is None
    if H == 24:
        assert pybert.test_cls_head(rows[:2, :20], Wp.astype(np.float16)[:20, :20], bp[:20], Wc[:, :20], bc, 0, "mfma") is None     # H = 20: not a multiple of 8


# ------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------
DIMS, e2e_batches = cer.DIMS, cer.e2e_batches
_FILES = {}


def _model_file(model_dir, dims, ftype, n_labels, seed=5):
    key = (dims, ftype, n_labels, seed)
    if key not in _FILES:
        path = os.path.join(model_dir, f"ce_{dims}_{ftype}_{n_labels}_{seed}.bin")
        gf.write_model(path, DIMS[dims], gf.synthetic_weights(DIMS[dims], seed, n_labels=n_labels), gf.FTYPE_BY_NAME[ftype])
        _FILES[key] = path
    return _FILES[key]


# ------------------------------------------------------------------------------------------------
# 3. nothing disturbed
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ["tiny", "tiny-h128", "minilm-l6"])
def test_untyped_calls_keep_their_bits(model_dir, dims):
    """The same encoder with and without a head: eval_packed returns equal bits; eval_packed_typed without first_len and with first_len =
    the lengths equals eval_packed under all four pooling x normalize settings; score_packed without first_len is the head hook applied to
    eval_packed's un-normalised [CLS] rows."""
    hp = DIMS[dims]
    plain, with_head = pybert.BertModel(_model_file(model_dir, dims, "f16", 0)), pybert.BertModel(_model_file(model_dir, dims, "f16", 3))
    assert plain.n_labels == 0 and with_head.n_labels == 3
    rng = np.random.default_rng(1)
    lens = [5, 33, 64, 1, 17] if dims != "minilm-l6" else [128, 5, 77, 128, 1]
    toks, cu, _, _ = cer.batch(rng, hp, [(n, max(1, n // 2)) for n in lens])
    for pooling in ("mean", "cls"):
        for normalize in ("1", "0"):
            for m in (plain, with_head):
                m.set_option("pooling", pooling); m.set_option("normalize", normalize)
            want = plain.eval_packed(toks, cu)
            assert np.isfinite(want).all() and _same(with_head.eval_packed(toks, cu), want)
            for m in (plain, with_head):
                assert _same(m.eval_packed_typed(toks, cu, None), want), (dims, pooling, normalize)
                assert _same(m.eval_packed_typed(toks, cu, np.diff(cu)), want), (dims, pooling, normalize)
    rows = with_head.eval_packed(toks, cu)                     # (pooling cls, normalize 0: the loop's last setting)
    raw = gf.read_model(_model_file(model_dir, dims, "f16", 3))
    Wp = np.frombuffer(raw.raw["pooler.dense.weight"][2], dtype=np.float16).reshape(hp.n_embd, hp.n_embd)
    bp, Wc, bc = (raw.dequantized(n) for n in ("pooler.dense.bias", "classifier.weight", "classifier.bias"))
    for sig in (False, True):
        assert _same(with_head.score_packed(toks, cu, None, sigmoid=sig), pybert.test_cls_head(rows, Wp, bp, Wc, bc, int(sig), "mfma"))
    plain.close(); with_head.close()


# ------------------------------------------------------------------------------------------------
# 4. end to end with types
# ------------------------------------------------------------------------------------------------
# The tolerance on the typed pass's un-normalised [CLS] rows, |row - float64| / max |row|: twice what the PARENT commit — which can only
# run these ids with type 0 everywhere — leaves between bert_hip_eval_packed (pooling cls, normalize 0) and the float64 model on the very
# batches below (profiles/cross_encoder_parity.txt, written by tools/cross_encoder_parity.py).  The arithmetic is the same and only the
# values differ: the factor covers the draw, not another mechanism.
PARENT_ROW_ERROR = {("tiny", "f32"): 1.097e-06, ("tiny", "f16"): 1.658e-03, ("tiny", "q4_0"): 1.946e-03, ("tiny-h128", "f16"): 1.699e-03,
                    ("minilm-l6", "f16"): 9.547e-04, ("minilm-l6", "q4_1"): 1.419e-03}
assert list(PARENT_ROW_ERROR) == cer.E2E_MODELS
@pytest.mark.parametrize("dims,ftype", list(PARENT_ROW_ERROR))
def test_typed_pass_and_scores_match_float64(model_dir, dims, ftype):
    """Typed passes end to end: the [CLS] rows within twice the parent's own error against float64, the scores within head_bound of the
    float64 scores given that row tolerance.  Small batches, a batch with sentences beyond a window, and 16 x 128 tokens (the one-launch
    route from the lane-order embedding)."""
    tol = 2 * PARENT_ROW_ERROR[(dims, ftype)]
    path = _model_file(model_dir, dims, ftype, 3)
    ref = cer.Model(path)
    m = pybert.BertModel(path)
    m.set_option("pooling", "cls"); m.set_option("normalize", "0")
    f32_route = ftype == "f32"
    for name, (toks, cu, fl, sents) in e2e_batches(dims).items():
        m.profile(True)
        rows = m.eval_packed_typed(toks, cu, fl).astype(np.float64)
        scores = m.score_packed(toks, cu, fl).astype(np.float64)
        names = set(m.profile_report())
        m.profile(False)
        assert "cls_head" in names and "embed_ln" in names, names
        if name == "full" and (dims, ftype) == ("minilm-l6", "f16"):
            assert "model_kernel" in names, names              # (full windows: it starts from the lane-order embedding kernel)
        want_rows = np.stack([ref.cls_row(s, int(f)) for s, f in zip(sents, fl)])
        scale = np.abs(want_rows).max(axis=1, keepdims=True)
        err = np.abs(rows - want_rows) / scale
        print(f"{dims} {ftype} {name}: worst |row - f64| / max |row| = {err.max():.3e} (allowed {tol:.3e})")
        assert err.max() <= tol, (dims, ftype, name, float(err.max()), tol)
        want = cer.head(want_rows, *ref.head_weights())
        bound = cer.head_bound(want_rows, tol * scale, *ref.head_weights(), mfma=not f32_route)
        serr = np.abs(scores - want)
        print(f"{dims} {ftype} {name}: worst score error / bound = {(serr / bound).max():.3e}")
        assert (serr <= bound).all(), (dims, ftype, name, float((serr / bound).max()))
        # types reach the model: the same ids with type 0 everywhere give other rows
        assert np.abs(m.eval_packed_typed(toks, cu, None) - rows).max() > 10 * tol * scale.max()
    m.close()


# ------------------------------------------------------------------------------------------------
# 5. text level, 6. errors
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_model(model_dir, tok_golden):
    """tiny dims over the golden tokenizer's vocabulary, with a head of one label"""
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    path = os.path.join(model_dir, "ce_text.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, n_labels=1), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return path, words


def test_score_pairs_and_rerank(text_model):
    path, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(3)
    docs = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=20)]
    query = " ".join(words[:4])
    pairs = [(query, d) for d in docs]
    got = m.score_pairs(pairs)
    ids = [m.tokenize_pair(a, b) for a, b in pairs]
    toks, cu, fl = np.concatenate([i for i, _ in ids]).astype(np.int32), _cu([len(i) for i, _ in ids]), [f for _, f in ids]
    assert got.shape == (20, 1) and _same(got, m.score_packed(toks, cu, fl))
    order, scores = m.rerank(query, docs, top_k=5)
    assert list(order) == sorted(range(20), key=lambda i: (-got[i, 0], i))[:5] and _same(scores, got[order, 0])
    swapped = m.score_pairs([(d, query) for d in docs])
    assert not np.array_equal(swapped, got) and np.abs(swapped - got).max() > 1e-3
    sig = m.score_pairs(pairs, sigmoid=True)
    assert np.allclose(sig, 1 / (1 + np.exp(-got.astype(np.float64))), atol=1e-6)
    m.close()


def test_errors(model_dir, capfd):
    hp = DIMS["tiny"]
    toks, cu, fl, _ = cer.batch(np.random.default_rng(0), hp, [(5, 2), (9, 9)])
    lib = pybert.lib()
    plain, with_head = pybert.BertModel(_model_file(model_dir, "tiny", "f16", 0)), pybert.BertModel(_model_file(model_dir, "tiny", "f16", 3))
    out = np.full((2, 3), 7.0, dtype=np.float32)
    i32p, f32p = pybert._i32p, pybert._f32p
    capfd.readouterr()
    assert lib.bert_hip_score_packed(plain.ctx, i32p(toks), i32p(cu), i32p(fl), 2, 0, f32p(out)) == -2
    assert "no classification head" in capfd.readouterr().err and (out == 7.0).all()
    assert lib.bert_hip_score_packed_device(plain.ctx, None, None, None, 2, 14, 9, 0, None, None) == -2
    assert "no classification head" in capfd.readouterr().err
    for bad in ([-1, 9], [2, 10]):
        b = np.array(bad, dtype=np.int32)
        assert lib.bert_hip_score_packed(with_head.ctx, i32p(toks), i32p(cu), i32p(b), 2, 0, f32p(out)) == -2
        assert "first_len" in capfd.readouterr().err and (out == 7.0).all()
        emb = np.full((2, hp.n_embd), 7.0, dtype=np.float32)
        assert lib.bert_hip_eval_packed_typed(with_head.ctx, i32p(toks), i32p(cu), i32p(b), 2, f32p(emb)) == -2 and (emb == 7.0).all()
    assert lib.bert_hip_score_packed(with_head.ctx, i32p(toks), i32p(cu), i32p(fl), 0, 0, f32p(out)) == 0 and (out == 7.0).all()
    assert lib.bert_hip_eval_packed_typed(with_head.ctx, i32p(toks), i32p(cu), None, -1, None) == 0
    assert lib.bert_hip_score_pairs(with_head.ctx, 1, 0, None, None, 0, None) == 0
    assert lib.bert_hip_score_packed(with_head.ctx, i32p(toks), i32p(cu), i32p(fl), 2, 0, f32p(out)) == 0 and np.isfinite(out).all()
    tok_only = pybert.BertModel(_model_file(model_dir, "tiny", "f16", 3), tokenizer_only=True)
    assert lib.bert_hip_score_packed(tok_only.ctx, i32p(toks), i32p(cu), i32p(fl), 2, 0, f32p(out)) == -1
    assert lib.bert_hip_eval_packed_typed(tok_only.ctx, i32p(toks), i32p(cu), i32p(fl), 2, f32p(out)) == -1
    assert lib.bert_hip_score_pairs(tok_only.ctx, 1, 1, None, None, 0, f32p(out)) == -1
    assert lib.bert_hip_score_packed_device(tok_only.ctx, None, None, None, 2, 14, 9, 0, None, None) == -1
    capfd.readouterr()
    for m in (plain, with_head, tok_only):
        m.close()


# ------------------------------------------------------------------------------------------------
# 7. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,batch", [("tiny", "short"), ("minilm-l6", "full")])
def test_score_packed_device_under_capture(model_dir, dims, batch):
    """After bert_hip_reserve, score_packed_device is captured and replayed twice: the eager call's bits, which are the host form's; an
    eager call afterwards still works."""
    hip = hip_graph.Hip()
    m = pybert.BertModel(_model_file(model_dir, dims, "f16", 3))
    toks, cu, fl, _ = e2e_batches(dims)[batch]
    B, T, max_len = len(cu) - 1, int(cu[-1]), int(np.diff(cu).max())
    host = m.score_packed(toks, cu, fl)
    d_t, d_cu, d_fl, d_out = hip.upload(toks), hip.upload(cu), hip.upload(fl), hip.nans((B, 3))
    s = hip.stream()
    m.reserve(T, B)
    lib = pybert.lib()

    def call():
        return lib.bert_hip_score_packed_device(m.ctx, d_t, d_cu, d_fl, B, T, max_len, 0, d_out, s)

    assert call() == 0
    eager = hip.download(d_out, (B, 3))
    assert m.check() == 0 and _same(eager, host)
    hip.poison(d_out, (B, 3))
    with hip.capture(s) as cap:
        r = call()
    assert r == 0 and cap.status == hip_graph.HIP_SUCCESS and cap.graph
    assert np.isnan(hip.download(d_out, (B, 3))).all(), "capturing must run nothing"
    assert hip.kernel_nodes(cap.graph) >= 3                    # (embedding, layers, head)
    ex = hip.instantiate(cap.graph)
    for i in range(2):
        hip.poison(d_out, (B, 3))
        hip.launch(ex, s)
        assert _same(hip.download(d_out, (B, 3)), eager), ("replay", i)
    hip.poison(d_out, (B, 3))
    assert call() == 0 and _same(hip.download(d_out, (B, 3)), eager) and m.check() == 0
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_fl, d_out)
    m.close()


# ------------------------------------------------------------------------------------------------
# 8. bert-search --cross-model
# ------------------------------------------------------------------------------------------------
def test_search_example_reranks_with_a_cross_encoder(text_model, tmp_path):
    """bert-search --cross-model ... --cross 5 on a 20-line file: k lines per query, in the order BertModel.rerank gives for the first
    stage's candidates, with its scores."""
    import subprocess
    from conftest import ROOT
    path, words = text_model
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    rng = np.random.default_rng(8)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(2, 30, size=20)]
    assert len(set(texts)) == 20
    file = tmp_path / "texts.txt"
    file.write_text("\n".join(texts) + "\n")
    queries = [" ".join(words[3:7]), texts[4]]
    r = subprocess.run([exe, "-m", path, "-f", str(file), "-k", "3", "--cross-model", path, "--cross", "5"], input="\n".join(queries) + "\nq\n",
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert "Loaded 20 lines." in r.stdout and len(blocks) == 2
    m = pybert.BertModel(path)
    ix = m.index()
    ix.add_texts(texts)
    cand, _ = ix.search_texts(queries, 5)
    for b, q, c in zip(blocks, queries, cand):
        order, scores = m.rerank(q, [texts[i] for i in c], top_k=3)
        lines = b.split("\n")
        for j in range(3):
            assert lines[2 * j] == f"{j + 1}. {texts[c[order[j]]]}", (lines, j)
            assert lines[2 * j + 1] == f" (cross-encoder score: {scores[j]:.4f})", (lines, j)
        assert not lines[6].startswith("4. ")
    m.close()
    # the flags' checks
    for args in (["--cross", "5"], ["--cross-model", path], ["--cross-model", path, "--cross", "2"], ["--cross-model", path, "--cross", "5", "--maxsim", "5"]):
        r = subprocess.run([exe, "-m", path, "-f", str(file), "-k", "3"] + args, input="q\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "search: --cross" in r.stderr, (args, r.stderr)
