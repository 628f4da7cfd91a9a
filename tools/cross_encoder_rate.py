#!/usr/bin/env python3
"""Rate of cross-encoder scoring (bert_hip_score_packed_device) on one GPU beside the untyped pass on the same ids
(bert_hip_eval_packed_device): what token types and the classification head cost.

    rerank   one query of 32 tokens against 1000 documents of 180 tokens: 1000 pairs of 32 + 180 = 212 ids ([CLS] q [SEP] d [SEP]),
             first_len 32, minilm-l6 dims with a head of one label, f16 file

    python tools/cross_encoder_rate.py [--iters 20] [--rounds 5] [--out profiles/cross_encoder_rate.txt]

Everything is in device memory; a figure is the time per call from device events around `iters` back-to-back calls on one stream (a
synchronise behind them), the median of `rounds` rounds, the two calls alternating round by round after warm-up calls.  The head's own
time is the profile's "cls_head" line of one profiled call."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cross_encoder_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ce.bin")
        hp = gf.MODEL_DIMS["minilm-l6"]
        gf.write_model(path, hp, gf.synthetic_weights(hp, 0, n_labels=1), gf.FTYPE_F16)
        m = pybert.BertModel(path)
        n_pairs, lq, ld = 1000, 32, 180
        L = lq + ld
        ids = gf.synthetic_token_ids(n_pairs, L, hp.n_vocab, seed=3)
        ids[:, lq - 1] = 102
        dev = torch.device("cuda")
        d_ids = torch.from_numpy(ids.reshape(-1)).to(dev)
        d_cu = (torch.arange(0, n_pairs + 1, dtype=torch.int32) * L).to(dev)
        d_fl = torch.full((n_pairs,), lq, dtype=torch.int32, device=dev)
        d_emb = torch.empty(n_pairs, hp.n_embd, dtype=torch.float32, device=dev)
        d_scores = torch.empty(n_pairs, 1, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        T = n_pairs * L
        m.reserve(T, n_pairs)

        def score():
            m.score_packed_device(d_ids.data_ptr(), d_cu.data_ptr(), d_fl.data_ptr(), n_pairs, T, L, d_scores.data_ptr(), False, stream)

        def embed():
            m.eval_packed_device(d_ids.data_ptr(), d_cu.data_ptr(), n_pairs, T, L, d_emb.data_ptr(), stream)

        for _ in range(2):
            score(); embed()
        torch.cuda.synchronize()
        assert m.check() == 0 and bool(torch.isfinite(d_scores).all()) and bool(torch.isfinite(d_emb).all())

        def timed(f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        t_s, t_e = [], []
        for _ in range(a.rounds):
            t_s.append(timed(score)); t_e.append(timed(embed))
        m.profile(True)
        score()
        torch.cuda.synchronize()
        rep = m.profile_report()
        m.profile(False)
        head_us = rep["cls_head"]["total_ms"] / max(rep["cls_head"]["launches"], 1) * 1e3 if "cls_head" in rep else float("nan")
        ms, me = float(np.median(t_s)), float(np.median(t_e))
        out(f"# bert_hip_score_packed_device beside bert_hip_eval_packed_device on the same ids, {torch.cuda.get_device_name(0)}; minilm-l6 dims, f16, "
            f"{n_pairs} pairs of {lq} + {ld} ids; ms per call = median of {a.rounds} rounds of {a.iters} calls between device events, the calls alternating")
        out("# call                          ms (min .. max)        pairs/s")
        out(f"  score_packed_device   {ms:9.3f} ({min(t_s):.3f} .. {max(t_s):.3f}) {n_pairs / ms * 1e3:12.0f}")
        out(f"  eval_packed_device    {me:9.3f} ({min(t_e):.3f} .. {max(t_e):.3f}) {n_pairs / me * 1e3:12.0f}")
        out(f"  types + head: {(ms - me) * 1e3:+.1f} us per call ({(ms / me - 1) * 100:+.2f} %); the cls_head launch alone, profiled: {head_us:.1f} us; kernels: {sorted(rep)}")
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
