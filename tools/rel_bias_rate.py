#!/usr/bin/env python3
"""What MPNet's relative position bias costs: the attention launch and the full forward pass of a model WITH the tensor beside the same
encoder WITHOUT it, in one process on one GPU, the two alternating.

    shapes   512 sentences x 128 tokens (the 4-wave one-chunk attention kernel) and 64 x 512 tokens (the 8-wave persistent one),
             12 heads x 64, mpnet-base dims (12 layers, H = 768): f16 and q4_0 files
    python tools/rel_bias_rate.py [--rounds 5] [--layers 12] [--out profiles/rel_bias_rate.txt]

Two figures per (file type, shape, model):
  attention  microseconds per attention launch by the engine's own profiler (bert_hip_profile_enable: device events around every launch,
             which serialises the pass): the median over --rounds profiled passes of total_ms / launches;
  pass       milliseconds per bert_hip_eval_packed call (blocking: ids in, pooled rows out; a host clock around a call that ends in a
             device synchronise), profiler off: the median, minimum and maximum over --rounds calls after two warm-up calls.
Both models take the same route here (H = 768 runs neither the fused projection + attention kernel nor the one-launch kernel), so the
difference is the bias: the table's staging, the LDS reads and the accumulators that start from them.  The models alternate call by
call; the spread of one model's own rounds is printed beside every difference."""
import argparse
import dataclasses
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    hp = dataclasses.replace(gf.MODEL_DIMS["mpnet-dims"], n_max_tokens=512, n_layer=a.layers)
    shapes = [(512, 128), (64, 512)]
    out(f"library {pybert.lib().bert_hip_version().decode()}; mpnet-base dims, {hp.n_layer} layers, H {hp.n_embd}, {hp.n_head} heads x {hp.n_embd // hp.n_head}; "
        f"{a.rounds} rounds, the two models alternating")
    with tempfile.TemporaryDirectory() as d:
        w = gf.synthetic_weights(hp, 1, rel_bias=True)
        plain = {k: v for k, v in w.items() if k != gf.REL_BIAS_NAME}
        for ftype in ("f16", "q4_0"):
            models = {}
            for name, weights in (("plain", plain), ("bias", w)):
                path = os.path.join(d, f"{name}_{ftype}.bin")
                gf.write_model(path, hp, weights, gf.FTYPE_BY_NAME[ftype], vocab=gf.synthetic_vocab(hp.n_vocab, mpnet=True))
                models[name] = pybert.BertModel(path)
            assert models["bias"].relative_attention and not models["plain"].relative_attention
            for B, n in shapes:
                toks = gf.synthetic_token_ids(B, n, hp.n_vocab, seed=3).reshape(-1).astype(np.int32)
                cu = (np.arange(B + 1) * n).astype(np.int32)
                att = {k: [] for k in models}
                wall = {k: [] for k in models}
                for m in models.values():
                    m.eval_packed(toks, cu); m.eval_packed(toks, cu)
                for _ in range(a.rounds):
                    for k, m in models.items():
                        t0 = time.perf_counter()
                        m.eval_packed(toks, cu)
                        wall[k].append((time.perf_counter() - t0) * 1e3)
                for _ in range(a.rounds):
                    for k, m in models.items():
                        m.profile(True)
                        m.eval_packed(toks, cu)
                        rep = m.profile_report()
                        m.profile(False)
                        assert rep["attention"]["launches"] == hp.n_layer and "qkv_attention2" not in rep and "model_kernel" not in rep, rep
                        att[k].append(rep["attention"]["total_ms"] * 1e3 / rep["attention"]["launches"])
                med = lambda v: statistics.median(v)
                for what, unit, v in (("attention", "us per launch", att), ("pass     ", "ms per call  ", wall)):
                    p, b = med(v["plain"]), med(v["bias"])
                    out(f"{ftype:5s} {B:4d} x {n:3d}  {what} {unit}: plain {p:9.2f} [{min(v['plain']):.2f} .. {max(v['plain']):.2f}]   "
                        f"bias {b:9.2f} [{min(v['bias']):.2f} .. {max(v['bias']):.2f}]   bias / plain {b / p:.3f}")
            for m in models.values():
                m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
