"""The projection head end to end (include/bert_hip.h "Projection head") on the tiny f16 model written with a random head, P = 32."""
import os
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from hip_graph import Hip

pytestmark = pytest.mark.gpu
P = 32
LENS = [1, 2, 17, 33, 48, 64]
WORDS = ["[PAD]", "[UNK]"] + [f"w{i}" for i in range(2, 101)] + ["[CLS]", "[SEP]", "hello", "world", "long", "text", "window", "index", "search", "row", ","]
DOCS = ["hello world", "text, window", "index search row", "long text window", "w5 w6 w7 w8 w9 w10 w11 w12", "search row index", "w7 " * 80, "hello hello"]
QUERIES = ["long text window", "hello", "index search w9"]

@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("token_proj")
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, seed=5)
    vocab = [t.encode() for t in WORDS] + [f"[unused{i}]".encode() for i in range(len(WORDS), hp.n_vocab)]
    gf.write_model(os.path.join(d, "plain.bin"), hp, w, gf.FTYPE_F16, vocab=vocab)
    w[gf.TOKEN_PROJ_NAME] = np.random.default_rng(5).normal(0, 1 / np.sqrt(hp.n_embd), (P, hp.n_embd)).astype(np.float32)
    gf.write_model(os.path.join(d, "colbert.bin"), hp, w, gf.FTYPE_F16, vocab=vocab)
    m, plain = pybert.BertModel(os.path.join(d, "colbert.bin")), pybert.BertModel(os.path.join(d, "plain.bin"))
    yield m, plain, hp, w[gf.TOKEN_PROJ_NAME].astype(np.float16)
    m.close(); plain.close()

def _batch(hp, lens=LENS, seed=400):
    sents = [gf.synthetic_token_ids(1, n, hp.n_vocab, seed=seed + i)[0] for i, n in enumerate(lens)]
    return sents, np.concatenate(sents).astype(np.int32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)

def test_rows_are_the_kernel_on_the_states_and_embeddings_keep_their_bits(models):
    m, plain, hp, wp = models
    assert m.token_dim == P and plain.token_dim == 0
    sents, toks, cu = _batch(hp)
    rows, emb = m.eval_packed_tokens(toks, cu, normalize=True, with_embeddings=True, project=True)
    states = m.eval_packed_tokens(toks, cu, normalize=False)                      # the stored f16 states, converted exactly
    assert rows.shape == (len(toks), P) and np.array_equal(states.astype(np.float16).astype(np.float32), states)
    want = pybert.test_token_project(states.astype(np.float16), wp, cu, max(LENS), True, False)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)) and np.isfinite(rows).all()
    assert np.array_equal(emb.view(np.uint32), m.eval_packed(toks, cu).view(np.uint32))
    # a sentence's projected rows: the same alone and in the batch
    for i in (0, 3, 5):
        alone = m.eval_packed_tokens(sents[i], np.array([0, len(sents[i])], np.int32), project=True)
        assert np.array_equal(alone.view(np.uint32), rows[cu[i]:cu[i + 1]].view(np.uint32))
    with pytest.raises(RuntimeError, match="-2"):                                # no head: the flag is an unknown one
        plain.eval_packed_tokens(toks, cu, project=True)
    assert np.isfinite(plain.eval_packed_tokens(toks, cu)).all()

def test_device_form_replays_under_capture(models):
    m, _, hp, _ = models
    hip = Hip()
    _, toks, cu = _batch(hp)
    _, toks2, _ = _batch(hp, seed=500)
    B, T = len(cu) - 1, len(toks)
    d_t, d_cu, d_rows, d_emb = hip.upload(toks), hip.upload(cu), hip.nans((T, P), np.float16), hip.nans((B, hp.n_embd))
    s = hip.stream()
    m.reserve(T, B)
    call = lambda: m.eval_packed_tokens_device(d_t, d_cu, B, T, max(LENS), d_rows, d_emb, normalize=True, f16=True, stream=s, project=True)
    call()
    assert np.array_equal(hip.download(d_rows, (T, P), np.float16).view(np.uint16), m.eval_packed_tokens(toks, cu, project=True).astype(np.float16).view(np.uint16))
    with hip.capture(s) as cap:
        call()
    assert cap.status == 0 and cap.graph
    ex = hip.instantiate(cap.graph)
    for ids in (toks, toks2, toks):
        hip.write(d_t, ids)
        hip.poison(d_rows, (T, P), np.float16)
        hip.launch(ex, s)
        got = hip.download(d_rows, (T, P), np.float16)
        assert np.array_equal(got.view(np.uint16), m.eval_packed_tokens(ids, cu, project=True).astype(np.float16).view(np.uint16))
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_rows, d_emb)

def test_token_index_at_the_heads_dim_from_texts(models):
    m = models[0]
    ix, twin = m.token_index(dim=P), m.token_index(dim=P)
    assert ix.add_texts(DOCS) == 0
    rows, cu = m.encode_tokens(DOCS, normalize=True, project=True)
    assert twin.add(rows, cu) == 0 and rows.shape[1] == P
    ids, scores = ix.search_texts(QUERIES, k=5)
    q_rows, q_cu = m.encode_tokens(QUERIES, normalize=True, project=True)
    want_ids, want_scores = twin.search(q_rows, q_cu, k=5)
    assert np.array_equal(ids, want_ids) and np.array_equal(scores.view(np.uint32), want_scores.view(np.uint32))
    assert np.isfinite(scores).all() and (ids >= 0).all()
    ix.close(); twin.close()
