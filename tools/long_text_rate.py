#!/usr/bin/env python3
"""Rate of the long-text path (bert_hip_encode_long_batch) on one GPU: texts/s and windows/s for synthetic texts of about 1000
tokens at windows of 128 and of 512 ids, host to host (tokenizing, the forward passes of every window, the grouped pooling, the
rows back in host memory), and — in a pass of its own, with the engine's per-kernel events on — the share of the pooling launch.

    python tools/long_text_rate.py [--texts 2048] [--tokens 1000] [--iters 5] [--out profiles/long_text_rate.txt]

The all-MiniLM-L6-v2 dimensions with seeded weights and a vocabulary of made-up words (the rate does not depend on the values)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_vocab(n_vocab, rng):
    """[PAD], [unused*], [UNK] [CLS] [SEP] [MASK] at their BERT ids, then made-up words of 2 .. 4 syllables, all different"""
    syll = ["ta", "re", "mo", "in", "ul", "es", "ka", "do", "vi", "ne", "or", "shi", "pla", "con", "ter", "ing", "ed", "ly", "un", "pre"]
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    seen = set(vocab)
    words = []
    while len(vocab) + len(words) < n_vocab:
        w = "".join(rng.choice(syll) for _ in range(int(rng.integers(2, 5))))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return vocab + words, words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=2048)
    ap.add_argument("--tokens", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--windows", default="128,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("long_text_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(1)
    hp = gf.MODEL_DIMS["minilm-l6"]
    vocab, words = make_vocab(hp.n_vocab, rng)
    # a text: whole vocabulary words, one id each: `tokens` - 2 words on average, +- 10 %
    texts = [" ".join(words[i] for i in rng.integers(0, len(words), int(rng.integers(int(0.9 * a.tokens), int(1.1 * a.tokens) + 1)) - 2))
             for _ in range(a.texts)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "minilm_words.bin")
        gf.write_model(path, hp, gf.synthetic_weights(hp, 1), gf.FTYPE_F16, vocab=[w.encode() for w in vocab])
        m = pybert.BertModel(path)
        n_ids = [len(m.tokenize_long(t)) for t in texts[:64]]
        out(f"# bert_hip_encode_long_batch, {a.texts} texts of {np.mean(n_ids):.0f} ids on average ({min(n_ids)} .. {max(n_ids)} among the first 64), "
            f"{torch.cuda.get_device_name(0)}, {a.threads} tokenizer threads; host to host, seconds per call = median of {a.iters} after 2 warm-up calls")
        out("# window stride | windows  windows/text |    s (min .. max)     texts/s   windows/s   tokens/s | group_pool: launches, ms, share of the kernels' time | model_kernel share")
        for window in (int(w) for w in a.windows.split(",")):
            window, stride = m.long_defaults(window, None)
            for _ in range(2):
                rows, nw = m.encode_long_batch(texts, window, stride, n_threads=a.threads, return_windows=True)
            assert np.isfinite(rows).all()
            secs = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                m.encode_long_batch(texts, window, stride, n_threads=a.threads)       # (blocking: the rows are in host memory when it returns)
                secs.append(time.perf_counter() - t0)
            med, W = float(np.median(secs)), int(nw.sum())
            # the per-kernel events in a call of their own (a timed launch runs behind fences: never inside the rate above)
            m.profile(True)
            m.encode_long_batch(texts, window, stride, n_threads=a.threads)
            prof = m.profile_report()
            m.profile(False)
            total = sum(k["total_ms"] for k in prof.values())
            gp = prof.get("group_pool", {"launches": 0, "total_ms": 0.0})
            mk = prof.get("model_kernel", {"total_ms": 0.0})
            out(f"  {window:5d} {stride:6d} | {W:7d} {W / a.texts:13.2f} | {med:6.3f} ({min(secs):.3f} .. {max(secs):.3f}) {a.texts / med:10.0f} {W / med:11.0f} "
                f"{W * window / med:10.0f} | {gp['launches']:3d} {gp['total_ms']:8.3f} ms {100 * gp['total_ms'] / max(total, 1e-9):6.2f} % | "
                f"{100 * mk['total_ms'] / max(total, 1e-9):6.2f} %")
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
