#!/usr/bin/env python3
"""Rate of the MaxSim kernel (bert_hip_maxsim_device) on one GPU beside torch's einsum + amax + sum on the same f16 rows:

    rerank   one query of 32 tokens against 1000 documents of 180 tokens, at H = 384 and at H = 768
    allpairs 256 queries x 256 documents of 25 tokens each, all pairs, at H = 384

    python tools/maxsim_rate.py [--iters 200] [--rounds 5] [--out profiles/maxsim_rate.txt]

Everything is in device memory; a figure is the time per call from device events around `iters` back-to-back calls on one stream
(a synchronise behind them), the median of `rounds` rounds, the two implementations alternating round by round after warm-up calls
of every shape.  torch scores a padded [docs, max_len, H] tensor (equal lengths here, so no padding is wasted and no mask is needed:
the comparison favours it); its output is checked against the kernel's within the reference's bound of the f32 chain.  FLOP/s counts
2 H per (query token, document token) product."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("maxsim_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)        # (a context to launch from: the kernel does not read the model)
        m = pybert.BertModel(path)
        dev = torch.device("cuda")
        gen = torch.Generator(device="cpu").manual_seed(1)
        out(f"# bert_hip_maxsim_device against torch einsum + amax + sum, f16 rows, {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
            f"us per call = median of {a.rounds} rounds of {a.iters} calls between device events, implementations alternating")
        out("# case                         H |  maxsim us (min .. max)   TFLOP/s |   torch us (min .. max)   TFLOP/s | torch / maxsim | max |diff|")
        cases = [("rerank 1x32 vs 1000x180", 384, 1, 32, 1000, 180), ("rerank 1x32 vs 1000x180", 768, 1, 32, 1000, 180), ("allpairs 256x25 vs 256x25", 384, 256, 25, 256, 25)]
        for name, H, n_q, lq, n_d, ld in cases:
            unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen), dim=1).to(torch.float16).to(dev)
            q, d = unit(n_q * lq), unit(n_d * ld)
            qcu = torch.arange(0, n_q + 1, dtype=torch.int32, device=dev) * lq
            dcu = torch.arange(0, n_d + 1, dtype=torch.int32, device=dev) * ld
            scores = torch.empty(n_q, n_d, dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            q3, d3 = q.view(n_q, lq, H), d.view(n_d, ld, H)

            def ours():
                m.maxsim_device(q.data_ptr(), qcu.data_ptr(), n_q, d.data_ptr(), dcu.data_ptr(), n_d, H, None, 0, scores.data_ptr(), False, stream)

            def theirs():
                return torch.einsum("aih,bjh->abij", q3, d3).amax(dim=3).sum(dim=2, dtype=torch.float32)

            for _ in range(3):
                ours(); ref = theirs()
            torch.cuda.synchronize()
            diff = float((scores - ref.float()).abs().max())
            assert diff < 2e-3 * lq, (name, H, diff)             # (torch rounds every product sum to f16 before the max)

            def timed(f):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.iters

            t_ours, t_theirs = [], []
            for _ in range(a.rounds):
                t_ours.append(timed(ours)); t_theirs.append(timed(theirs))
            flops = 2.0 * H * n_q * lq * n_d * ld
            mo, mt = float(np.median(t_ours)), float(np.median(t_theirs))
            out(f"  {name:28s} {H:4d} | {mo:9.1f} ({min(t_ours):.1f} .. {max(t_ours):.1f}) {flops / mo * 1e-6:9.2f} | {mt:9.1f} ({min(t_theirs):.1f} .. {max(t_theirs):.1f}) "
                f"{flops / mt * 1e-6:9.2f} | {mt / mo:14.2f} | {diff:.2e}")
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
