"""GPU tests of the relative position bias (MPNet models): the attention kernels at op level against the float64 attention with the bias
(rel_bias_reference.py), what pins the lookup (W = 0, a constant per head, poisoned neighbours), whole models end to end against the
float64 model on every route they can take, the routes they must not take, and the text entry points."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import rel_bias_reference as rb
from hip_graph import Hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = rb.P_OP
N_HEAD = 2
NAN16 = 0x7E00
IMPL = {"mfma": 0, "naive": 1}


def _worst(got, want, bnd):
    return float((np.abs(got.astype(np.float64) - want) / bnd).max())


def _per_sentence(frac_of, lens):
    t0, out = 0, {}
    for n in lens:
        out[n] = frac_of(slice(t0, t0 + n))
        t0 += n
    return out


# ------------------------------------------------------------------------------------------------
# 1. op level
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", ["mfma", "naive"])
def test_attention_with_the_bias_is_within_its_bound(kind, d_head):
    """One batch of all of LENS — the bucket edges, the full one-chunk form, the persistent walk over items of different length and
    head — under W ~ N(0, 2^2), against the float64 attention within the kernel's derived bound."""
    W, want, bnd = rb.op_reference(rb.LENS, N_HEAD, d_head, kind)
    got = pybert.test_attention_bias(rb.op_inputs(rb.LENS, N_HEAD, d_head), rb.cu_of(rb.LENS), N_HEAD, d_head, IMPL[kind], W, P)
    frac = _per_sentence(lambda s: _worst(got[s], want[s], bnd[s]), rb.LENS)
    print(f"\n{kind} d_head {d_head}: worst fraction of the bound per length {({n: round(f, 3) for n, f in frac.items()})}")
    assert max(frac.values()) <= 1.0, frac


@pytest.mark.parametrize("d_head", [32, 64])
def test_f32_attention_with_the_bias_is_within_its_bound(d_head):
    W, want, bnd = rb.op_reference(rb.LENS, N_HEAD, d_head, "f32")
    qkv = rb.op_inputs(rb.LENS, N_HEAD, d_head).astype(np.float32)
    got = pybert.test_f32_attention_bias(qkv, rb.cu_of(rb.LENS), N_HEAD, d_head, max(rb.LENS), W, P)
    frac = _per_sentence(lambda s: _worst(got[s], want[s], bnd[s]), rb.LENS)
    print(f"\nf32 d_head {d_head}: worst fraction of the bound per length {({n: round(f, 3) for n, f in frac.items()})}")
    assert max(frac.values()) <= 1.0, frac


@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", ["mfma", "naive"])
def test_a_zero_table_gives_the_bits_without_one(kind, d_head):
    """s + 0 is s: everything but the lookup is the kernel without the bias"""
    qkv, cu = rb.op_inputs(rb.LENS, N_HEAD, d_head), rb.cu_of(rb.LENS)
    plain = pybert.test_attention(qkv, cu, N_HEAD, d_head, IMPL[kind])
    zero = pybert.test_attention_bias(qkv, cu, N_HEAD, d_head, IMPL[kind], np.zeros((32, N_HEAD), dtype=np.float32), P)
    assert np.array_equal(plain.view(np.uint16), zero.view(np.uint16))
    # and each length alone (the one-chunk form for every sentence up to 128 tokens, which the batch above runs in the persistent one)
    t0 = 0
    for n in rb.LENS:
        one = pybert.test_attention_bias(qkv[t0:t0 + n], rb.cu_of([n]), N_HEAD, d_head, IMPL[kind], np.zeros((32, N_HEAD), dtype=np.float32), P)
        alone = pybert.test_attention(qkv[t0:t0 + n], rb.cu_of([n]), N_HEAD, d_head, IMPL[kind])
        assert np.array_equal(one.view(np.uint16), alone.view(np.uint16)), n
        t0 += n


@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", ["mfma", "naive"])
def test_a_constant_per_head_changes_nothing(kind, d_head):
    """softmax is shift-invariant: W[:, h] = c_h stays within the bound of the float64 result WITHOUT a bias"""
    qkv, cu = rb.op_inputs(rb.LENS, N_HEAD, d_head), rb.cu_of(rb.LENS)
    W = np.tile(np.array([3.25, -1.5], dtype=np.float32), (32, 1))
    _, bnd = rb.attention_packed(qkv, rb.LENS, N_HEAD, d_head, W, kind)            # (the bound knows the magnitude that was added)
    want, _ = rb.attention_packed(qkv, rb.LENS, N_HEAD, d_head, None, kind)
    got = pybert.test_attention_bias(qkv, cu, N_HEAD, d_head, IMPL[kind], W, P)
    assert _worst(got, want, bnd) <= 1.0


@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", ["mfma", "naive"])
def test_loud_neighbours(kind, d_head):
    """NaN rows behind the tokens and NaN table entries outside [P - n, P + n - 2]: a sentence of n tokens reads neither.  One launch
    per length (the window is the sentence's own), and the mixed batch with the rows behind it poisoned."""
    W = rb.draw_W(N_HEAD)
    scale = np.sqrt(d_head) if kind == "mfma" else 1.0
    table = (rb.rel_table(W, P).astype(np.float64) * scale).astype(np.float32)
    qkv, cu = rb.op_inputs(rb.LENS, N_HEAD, d_head), rb.cu_of(rb.LENS)
    clean = pybert.test_attention_bias(qkv, cu, N_HEAD, d_head, IMPL[kind], W, P)
    with pybert.test_pad(NAN16, 0x7FC00000):
        loud = pybert.test_attention_bias(qkv, cu, N_HEAD, d_head, IMPL[kind], W, P)
    assert np.array_equal(clean.view(np.uint16), loud.view(np.uint16))
    t0 = 0
    for n in rb.LENS:
        poisoned = np.full_like(table, np.nan)
        poisoned[:, P - n:P + n - 1] = table[:, P - n:P + n - 1]
        q1, cu1 = qkv[t0:t0 + n], rb.cu_of([n])
        want = pybert.test_attention_bias(q1, cu1, N_HEAD, d_head, IMPL[kind], None, P, rel=table)
        with pybert.test_pad(NAN16, 0x7FC00000):
            got = pybert.test_attention_bias(q1, cu1, N_HEAD, d_head, IMPL[kind], None, P, rel=poisoned)
        assert not np.isnan(got).any() and np.array_equal(got.view(np.uint16), want.view(np.uint16)), n
        t0 += n


# ------------------------------------------------------------------------------------------------
# 2. end to end
# ------------------------------------------------------------------------------------------------
# The tolerance on |row - float64| / max |row|, for the pooled rows of eval_packed and for the hidden states of every layer: twice what
# the PARENT commit's library leaves on the same encoder weights WITHOUT the tensor against the same float64 model with W = 0, on the
# same sentences.  Measured on an MI355X on 2026-10-21 with the parent's libbert.so by
#     python tools/rel_bias_parent.py --parent <bert.cpp_amd of a built parent checkout>      (it prints these two dictionaries and the
# digests further down; profiles/rel_bias_parent.txt is its output)
# The feature adds one f32 add per score; a wrong bucket under N(0, 2^2) weights misses these by orders of magnitude.
PARENT_POOLED_ERROR = {"h64-f32": 6.329e-07, "h64-f16": 9.993e-04, "h64-q4_0": 8.438e-04, "h768-f16": 9.696e-04}
PARENT_HIDDEN_ERROR = {"h64-f32": 1.803e-06, "h64-f16": 2.692e-03, "h64-q4_0": 2.595e-03, "h768-f16": 1.819e-03}
E2E_ROUTE = {"h64-f32": "f32", "h64-f16": "layered", "h64-q4_0": "layered", "h768-f16": "folded"}


def e2e_file(model_dir, name, rel_bias=True):
    hp, ftype, _ = rb.E2E_MODELS[name]
    path = os.path.join(model_dir, f"relbias_{name}_{int(rel_bias)}.bin")
    if not os.path.exists(path):
        gf.write_model(path, hp, gf.synthetic_weights(hp, rb.E2E_SEED, rel_bias=rel_bias), gf.FTYPE_BY_NAME[ftype])
    return path


def _launches(m, fn):
    m.profile(True)
    fn()
    rep = {k: v["launches"] for k, v in m.profile_report(families=True).items()}
    m.profile(False)
    return rep


@pytest.mark.parametrize("name", list(rb.E2E_MODELS))
def test_models_match_float64_end_to_end(model_dir, name):
    path = e2e_file(model_dir, name)
    ref = rb.Model(path)
    m = pybert.BertModel(path)
    assert m.relative_attention
    sents = rb.e2e_sentences(name)
    cu = rb.cu_of([len(s) for s in sents])
    rep = _launches(m, lambda: m.eval_packed(np.concatenate(sents), cu))
    got = m.eval_packed(np.concatenate(sents), cu)
    hid = [ref.hidden(s) for s in sents]
    want = np.stack([h[-1].mean(axis=0) / np.linalg.norm(h[-1].mean(axis=0)) for h in hid])
    e_pool = rb.row_error(got, want)
    e_hid = max(rb.row_error(m.eval_hidden(s)[1], h) for s, h in zip(sents, hid))
    print(f"\n{name}: pooled {e_pool:.3e} (parent {PARENT_POOLED_ERROR[name]}), hidden {e_hid:.3e} (parent {PARENT_HIDDEN_ERROR[name]}); launches {rep}")
    # the route: the f32 kernels for the f32 file; LayerNorm folding on gemm256 at H = 768; never a kernel with an attention of its own
    assert rep.get("attention", 0) == ref.hp.n_layer and not any(k in rep for k in ("qkv_attention2", "model_kernel")), rep
    assert ("family:gemm_f32" in rep) == (E2E_ROUTE[name] == "f32") and ("ln_rows_finalize" in rep) == (E2E_ROUTE[name] == "folded"), rep
    assert e_pool <= 2 * PARENT_POOLED_ERROR[name] and e_hid <= 2 * PARENT_HIDDEN_ERROR[name]
    m.close()


def test_a_bias_model_takes_no_kernel_with_an_attention_of_its_own(model_dir):
    """H = 384 / 12 heads, sentences of up to 128 tokens: without the tensor the fused projection + attention kernel, the one-launch
    kernel (full windows) and the latency route (a small call) serve this shape; with it none of them does."""
    hp = gf.BertHParams(512, 512, 384, 1536, 12, 2)
    paths = {}
    for rel in (False, True):
        paths[rel] = os.path.join(model_dir, f"relbias_h384_{int(rel)}.bin")
        gf.write_model(paths[rel], hp, gf.synthetic_weights(hp, 2, rel_bias=rel), gf.FTYPE_F16)
    rng = np.random.default_rng(5)
    batches = {"full windows": [128] * 16, "mixed": [5, 64, 128, 33] * 6, "one short sentence": [40]}
    fused = ("qkv_attention2", "model_kernel", "skinny_qkv", "skinny_proj", "skinny_ffn_up", "skinny_ffn_down", "skinny_layernorm")
    seen = set()
    for rel in (False, True):
        m = pybert.BertModel(paths[rel])
        m.set_option("latency_tokens", "768")                 # (the shipped default; the test session caps it at one window)
        ref = rb.Model(paths[rel])
        for what, lens in batches.items():
            sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in lens]
            rep = _launches(m, lambda: m.eval_packed(np.concatenate(sents), rb.cu_of(lens)))
            used = {k for k in fused if k in rep}
            if rel:
                assert not used and rep.get("attention", 0) == hp.n_layer, (what, rep)
                got = m.eval_packed(np.concatenate(sents[:2]), rb.cu_of(lens[:2]))
                assert rb.row_error(got, np.stack([ref.pooled(s) for s in sents[:2]])) < 1e-2, what
            else:
                seen |= used
        m.close()
    assert {"qkv_attention2", "model_kernel", "skinny_qkv"} <= seen, seen      # the shape does take them without the tensor


# A BERT file keeps its bits: sha256 of eval_packed's rows on two files without the tensor, recorded from the PARENT commit's library in
# the session that measured the tolerances above (tools/rel_bias_parent.py): the one-launch route and the folded one.
PARENT_BITS = {"one-launch": "4267d33cfec7a06d8e99338a8e89b801103bb62e3dd5441ce21e9994b1eedde4",
               "folded": "800be8a946e3a96acfe0a1097b4ded88357caa5b794e5592bd467e744115693a"}
BITS_MODELS = {"one-launch": (gf.MODEL_DIMS["minilm-l6"], "f16", [128] * 16), "folded": (gf.BertHParams(512, 512, 768, 3072, 12, 2), "f16", [128, 64, 300, 17])}


def bits_case(model_dir, which):
    hp, ftype, lens = BITS_MODELS[which]
    path = os.path.join(model_dir, f"relbias_bits_{which}.bin")
    if not os.path.exists(path):
        gf.write_model(path, hp, gf.synthetic_weights(hp, 1), gf.FTYPE_BY_NAME[ftype])
    rng = np.random.default_rng(17)
    sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in lens]
    return path, np.concatenate(sents), rb.cu_of(lens)


@pytest.mark.parametrize("which", list(PARENT_BITS))
def test_a_bert_file_keeps_its_bits(model_dir, which):
    path, toks, cu = bits_case(model_dir, which)
    m = pybert.BertModel(path)
    assert not m.relative_attention
    rep = _launches(m, lambda: m.eval_packed(toks, cu))
    assert ("model_kernel" in rep) == (which == "one-launch") and ("ln_rows_finalize" in rep) == (which == "folded"), rep
    assert hashlib.sha256(m.eval_packed(toks, cu).tobytes()).hexdigest() == PARENT_BITS[which]
    m.close()


# ------------------------------------------------------------------------------------------------
# 3. capture, texts, pairs, bert-search
# ------------------------------------------------------------------------------------------------
def test_capture_and_replay(model_dir):
    path = e2e_file(model_dir, "h64-f16")
    m = pybert.BertModel(path)
    sents = rb.e2e_sentences("h64-f16")[2:9]
    toks, cu = np.concatenate(sents), rb.cu_of([len(s) for s in sents])
    B, T, H, max_len = len(sents), int(cu[-1]), m.n_embd, int(np.diff(cu).max())
    host = m.eval_packed(toks, cu)
    hip = Hip()
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.nans((B, H))
    s = hip.stream()
    m.reserve(T, B)
    call = lambda: pybert.lib().bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max_len, d_out, s)
    assert call() == 0
    assert np.array_equal(hip.download(d_out, (B, H)), host)
    with hip.capture(s) as cap:
        r = call()
    assert r == 0 and cap.status == 0 and cap.graph
    ex = hip.instantiate(cap.graph)
    for _ in range(2):
        hip.poison(d_out, (B, H))
        hip.launch(ex, s)
        assert np.array_equal(hip.download(d_out, (B, H)), host)
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_out)
    m.close()


WORDS = ["<s>", "<pad>", "</s>", "<unk>"] + list("abcdefghij") + ["hello", "world", "##ing", "##s", "test", ",", ".", "!", "embed", "##ding", "search", "text"]


@pytest.fixture(scope="module")
def text_model(tmp_path_factory):
    hp = gf.MODEL_DIMS["tiny-h128"]
    vocab = [w.encode() for w in WORDS] + [f"[unused{i}]".encode() for i in range(len(WORDS), hp.n_vocab)]
    path = str(tmp_path_factory.mktemp("relbias") / "text_model.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, n_labels=1, rel_bias=True), gf.FTYPE_F16, vocab=vocab)
    return path


def test_encode_batch_wraps_texts_in_the_files_ids(text_model):
    m = pybert.BertModel(text_model)
    texts = ["hello world", "testing embeddings, hello!", "a b c d e f g h i j " * 5, ""]
    ids = [m.tokenize(t) for t in texts]
    assert all(i[0] == 0 and i[-1] == 2 for i in ids) and ids[0] == [0, WORDS.index("hello"), WORDS.index("world"), 2]
    got = m.encode_batch(texts)
    want = m.eval_packed(np.concatenate(ids).astype(np.int32), rb.cu_of([len(i) for i in ids]))
    assert np.array_equal(got, want)
    ref = rb.Model(text_model)
    assert rb.row_error(got, np.stack([ref.pooled(i) for i in ids])) < 1e-2
    m.close()


def test_text_pairs_are_refused(text_model, capfd):
    m = pybert.BertModel(text_model)
    assert m.n_labels == 1
    scores = np.zeros((1, 1), dtype=np.float32)
    import ctypes as C
    ta, tb = (C.c_char_p * 1)(b"hello"), (C.c_char_p * 1)(b"world")
    capfd.readouterr()
    r = pybert.lib().bert_hip_score_pairs(m.ctx, 1, 1, ta, tb, 0, scores.ctypes.data_as(C.POINTER(C.c_float)))
    assert r == -2 and "relative position bias" in capfd.readouterr().err
    # the packed route takes ids as given
    ids = np.array([0, 14, 2, 2, 15, 2], dtype=np.int32)
    assert np.isfinite(m.score_packed(ids, rb.cu_of([6]), None)).all()
    m.close()


def test_bert_search_returns_its_own_lines_first(text_model, tmp_path):
    lines = ["hello world", "testing embeddings", "a b c d", "search text, hello!", "j i h g f e"]
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    asked = [lines[1], lines[4]]
    r = subprocess.run([exe, "-m", text_model, "-f", str(f), "-k", "2"], input="".join(q + "\n" for q in asked) + "q\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert len(blocks) == 2
    for b, q in zip(blocks, asked):
        assert q in b.splitlines()[0], (q, b)
