#!/usr/bin/env python3
"""Rate of the token index's int8 form (bert_hip_late_index_create with dtype 2) beside the f16 form, both built from the same f16 rows
in the same process on one GPU:

    workloads (queries of 32 tokens, k = 10; 1, 8 and 64 queries), at dim 384 and at dim 128:
      scan     10^5 documents of 180 tokens and 10^6 documents of 25 tokens, generated on the device
      rescore  1000 candidates per query over the same indexes

    python tools/late_i8_rate.py [--scale 1.0] [--rounds 3] [--budget-ms 300] [--out profiles/late_i8_rate.txt]

Everything is in device memory; a figure is the time per call from device events around back-to-back calls on one stream (as many as
fit --budget-ms, at least 2, after a warm-up call of either index), the median of --rounds rounds, the two indexes alternating within
each round.  --scale shrinks the document counts (a smoke run).  Per workload the stored bytes of both forms (2 dim against dpad + 4 per
token, the lengths apart) and, per search, the overlap of the two indexes' top-10 ids — the quality figure: the int8 index answers under
its own score, not the f16 one's.  A scan's line also states the int8 form's share of the HBM line: n_tokens (dpad + 4) bytes per QUERY
over the time against 8.0 TB/s."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("late_i8_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def measure(impls):
        """impls: name -> callable; us per call: (median, min, max) per name, alternating within each round"""
        iters = {}
        for name, f in impls.items():
            f(); torch.cuda.synchronize()
            once = timed(f, 1)
            iters[name] = int(max(2, min(200, a.budget_ms * 1e3 / max(once, 1.0))))
        t = {name: [] for name in impls}
        for _ in range(a.rounds):
            for name, f in impls.items():
                t[name].append(timed(f, iters[name]))
        return {name: (float(np.median(v)), min(v), max(v)) for name, v in t.items()}

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)        # (a context to launch from: the kernels do not read the model)
        m = pybert.BertModel(path)
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(1)
        lq, k, n_cand = 32, 10, 1000
        out(f"# token index, int8 form beside the f16 form on the same f16 rows, queries of {lq} tokens, k = {k}; {torch.cuda.get_device_name(0)}, "
            f"torch {torch.__version__}; us per call = median (min .. max) of {a.rounds} rounds between device events, the two indexes alternating; "
            f"scale {a.scale}; a ratio below 1 (int8 slower) is marked **")
        out("# case                                   dim   nq |     f16 us (min .. max) |    int8 us (min .. max) | f16 / int8 | top-10 overlap | int8 HBM share")
        stream = torch.cuda.current_stream().cuda_stream
        for H in (384, 128):
            dpad = (H + 31) // 32 * 32
            unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
            for n_docs, ld in ((int(100000 * a.scale), 180), (int(1000000 * a.scale), 25)):
                n_tok = n_docs * ld
                d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
                for t0 in range(0, n_tok, 1 << 20):
                    d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
                dcu_h = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
                index = {}
                for name in ("f16", "i8"):
                    ix = m.token_index(H, name)
                    ix.reserve(n_docs, n_tok, 64, lq, k)
                    assert ix.add_device(dcu_h, d.data_ptr(), stream) == 0
                    index[name] = ix
                torch.cuda.synchronize()
                b16, b8 = n_tok * 2 * H, n_tok * (dpad + 4)
                out(f"  stored {n_docs:8d} x {ld:3d} tokens, dim {H}: f16 {b16 / 1e9:.2f} GB, int8 {b8 / 1e9:.2f} GB, int8 / f16 = {b8 / b16:.3f} "
                    f"((dpad + 4) / (2 dim) = {(dpad + 4) / (2 * H):.3f})")
                for nq in (1, 8, 64):
                    q = unit(nq * lq)
                    qcu = torch.arange(0, nq + 1, dtype=torch.int32, device=dev) * lq
                    res = {name: (torch.empty(nq, k, dtype=torch.int32, device=dev), torch.empty(nq, k, dtype=torch.float32, device=dev)) for name in index}

                    def scan(name):
                        return lambda: index[name].search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, res[name][0].data_ptr(), res[name][1].data_ptr(), stream)

                    def overlap():
                        torch.cuda.synchronize()
                        a16, a8 = res["f16"][0].cpu().numpy(), res["i8"][0].cpu().numpy()
                        return float(np.mean([len(set(x[x >= 0]) & set(y[y >= 0])) / max(1, int((x >= 0).sum())) for x, y in zip(a16, a8)]))

                    def line(what, t, hbm):
                        r = t["f16"][0] / t["i8"][0]
                        mark = "**" if r < 1.0 else "  "
                        out(f"  {what:36s} {H:5d} {nq:4d} | {t['f16'][0]:10.1f} ({t['f16'][1]:.1f} .. {t['f16'][2]:.1f}) | {t['i8'][0]:10.1f} ({t['i8'][1]:.1f} .. {t['i8'][2]:.1f}) | "
                            f"{mark}{r:6.2f}{mark} | {overlap():14.3f} | {hbm}")

                    t = measure({"f16": scan("f16"), "i8": scan("i8")})
                    line(f"scan {n_docs:8d} x {ld:3d} tokens", t, f"{nq * b8 / (t['i8'][0] * 1e-6) / 1e12 / HBM_TBS:.3f}")

                    nc = min(n_cand, n_docs)
                    cand = torch.randint(0, n_docs, (nq, nc), generator=gen, device=dev, dtype=torch.int32)

                    def rescore(name):
                        return lambda: index[name].rescore_device(nq, qcu.data_ptr(), q.data_ptr(), nc, cand.data_ptr(), k, res[name][0].data_ptr(), res[name][1].data_ptr(), stream)

                    t = measure({"f16": rescore("f16"), "i8": rescore("i8")})
                    line(f"rescore {nc:5d} of {n_docs:8d} x {ld:3d}", t, "-")
                for ix in index.values():
                    ix.close()
                del d
                torch.cuda.empty_cache()
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
