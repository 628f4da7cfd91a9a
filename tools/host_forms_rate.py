#!/usr/bin/env python3
"""Time per call of the engine's blocking host forms and of the indexes' text routes, on one GPU, for comparing two builds of the
library process by process (BERT_HIP_LIB selects the build; profiles/host_forms_rate.txt alternates the parent commit's and this one's).

    python tools/host_forms_rate.py [--runs 5] [--json FILE]

minilm-l6 dims, f16 file with a 3-label head and the MLM head.  A cell is a blocking call on host memory under a host clock: the median
of `runs` runs, ms per call.  `_cut`: the same call under chunk_tokens = 4096, so that it goes through the chunk walk and the staging of a
chunk several times.
  typed / score        eval_packed_typed / score_packed, 256 pairs of 128 tokens
  tokens               eval_packed_tokens, 128 sentences of 64 tokens (rows f32, with embeddings)
  sparse_top64         sparse_packed k = 64, 1024 sentences of 25 tokens
  sparse_dense         sparse_packed k = None, 64 sentences of 25 tokens
  late_search_texts    token index of 2000 texts, search_texts of 512 queries of 4 .. 10 words, k = 10
  sparse_search_texts  sparse index (width 128, f32) of 2000 texts, search_texts of 512 queries, kq = 32, k = 10"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    hp = gf.MODEL_DIMS["minilm-l6"]
    rng = random.Random(1)
    syll = ["ta", "re", "mo", "in", "ul", "es", "ka", "do", "vi", "ne", "or", "shi", "pla", "con", "ter", "ing", "ed", "ly", "un", "pre"]
    words = sorted({"".join(rng.choice(syll) for _ in range(rng.randint(1, 4))) for _ in range(6000)})
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words
    vocab += [f"[unused{i}]" for i in range(len(vocab), hp.n_vocab)]
    texts = [" ".join(rng.choice(words) for _ in range(rng.randint(5, 40))) for _ in range(2000)]
    queries = [" ".join(rng.choice(words) for _ in range(rng.randint(4, 10))) for _ in range(512)]

    def batch(B, L, seed):
        return gf.synthetic_token_ids(B, L, hp.n_vocab, seed=seed).reshape(-1).astype(np.int32), (np.arange(B + 1) * L).astype(np.int32)

    cells = {}

    def cell(name, f, calls):
        f()
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            runs.append((time.perf_counter() - t0) / calls * 1e3)
        cells[name] = float(np.median(runs))
        print(f"{name:28s} {cells[name]:10.3f} ms per call", flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "host_forms.bin")
        gf.write_model(path, hp, gf.synthetic_weights(hp, 0, n_labels=3, mlm_head=True), gf.FTYPE_F16, vocab=[v.encode() for v in vocab[:hp.n_vocab]])
        m = pybert.BertModel(path)
        toks, cu = batch(256, 128, 3)
        fl = np.full(256, 32, dtype=np.int32)
        t_toks, t_cu = batch(128, 64, 4)
        s_toks, s_cu = batch(1024, 25, 5)
        late = m.token_index()
        late.add_texts(texts)
        sparse = m.sparse_index(128, "f32")
        sparse.add_texts(texts)
        for suffix, chunk_tokens in (("", "262144"), ("_cut", "4096")):
            m.set_option("chunk_tokens", chunk_tokens)
            cell("typed" + suffix, lambda: m.eval_packed_typed(toks, cu, fl), 10)
            cell("score" + suffix, lambda: m.score_packed(toks, cu, fl), 10)
            cell("tokens" + suffix, lambda: m.eval_packed_tokens(t_toks, t_cu, normalize=True, with_embeddings=True), 10)
            cell("sparse_top64" + suffix, lambda: m.sparse_packed(s_toks, s_cu, 64), 5)
            cell("sparse_dense" + suffix, lambda: m.sparse_packed(s_toks[:64 * 25], s_cu[:65]), 10)
            cell("late_search_texts" + suffix, lambda: late.search_texts(queries, 10), 5)
            cell("sparse_search_texts" + suffix, lambda: sparse.search_texts(queries, 32, 10), 5)
        m.set_option("chunk_tokens", "262144")
        late.close(); sparse.close(); m.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(cells, f)


if __name__ == "__main__":
    main()
