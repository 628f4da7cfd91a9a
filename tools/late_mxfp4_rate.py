#!/usr/bin/env python3
"""Rate of the token index's MXFP4 form (bert_hip_late_index_create with dtype 4) beside the int8 and f16 forms, all three built from
the same f16 rows in one process on one GPU — tools/late_i8_rate.py's workloads (queries of 32 tokens, k = 10; 1, 8 and 64 queries; dim
384 and 128; 10^5 documents of 180 tokens and 10^6 of 25; a rescore of 1000 candidates):

    python tools/late_mxfp4_rate.py [--scale 1.0] [--rounds 5] [--budget-ms 150] [--out profiles/late_mxfp4_rate.txt]

Per workload the MXFP4 index is first held against itself (a query alone against the batch, a rescore of the search's ids against the
search: ids and bits).  A figure is the time per call from device events around back-to-back calls on one stream, the FASTEST of --rounds
rounds with (min .. max), the three indexes alternating within each round.  A scan's share of the HBM line: the form's stored bytes
per query over the time against 8.0 TB/s.  Quality: the overlap of each form's top-10 ids with the f16 form's on these random unit rows."""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0
FORMS = ("f16", "i8", "mxfp4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-ms", type=float, default=150.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("late_mxfp4_rate.py needs a GPU")
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
        """us per call, (fastest, slowest) of the rounds per name, the names alternating within each round"""
        iters = {}
        for name, f in impls.items():
            f(); torch.cuda.synchronize()
            iters[name] = int(max(2, min(200, a.budget_ms * 1e3 / max(timed(f, 1), 1.0))))
        t = {name: [] for name in impls}
        for _ in range(a.rounds):
            for name, f in impls.items():
                t[name].append(timed(f, iters[name]))
        return {name: (min(v), max(v)) for name, v in t.items()}

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)        # (a context to launch from: the kernels do not read the model)
        m = pybert.BertModel(path)
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(1)
        lq, k, n_cand = 32, 10, 1000
        stream = torch.cuda.current_stream().cuda_stream
        out(f"# token index: f16, int8 and mxfp4 forms on the same f16 rows, queries of {lq} tokens, k = {k}; {torch.cuda.get_device_name(0)}, torch "
            f"{torch.__version__}; us per call = fastest (.. slowest) of {a.rounds} rounds between device events, the indexes alternating; scale {a.scale}; "
            f"a ratio below 1 (mxfp4 slower) is marked **")
        out("# case                                   dim   nq |  f16 us (.. max) | int8 us (.. max) | mxfp4 us (.. max) | f16 / mx | int8 / mx | top-10 overlap with f16: int8, mxfp4 | HBM share f16, int8, mxfp4")
        for H in (384, 128):
            row = {"f16": 2 * H, "i8": (H + 31) // 32 * 32 + 4, "mxfp4": ((H + 63) // 64 * 64 * 17 // 32 + 15) // 16 * 16}
            unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
            for n_docs, ld in ((int(100000 * a.scale), 180), (int(1000000 * a.scale), 25)):
                n_tok = n_docs * ld
                d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
                for t0 in range(0, n_tok, 1 << 20):
                    d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
                dcu_h = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
                index = {}
                for name in FORMS:
                    index[name] = m.token_index(H, name)
                    index[name].reserve(n_docs, n_tok, 64, lq, k)
                    assert index[name].add_device(dcu_h, d.data_ptr(), stream) == 0
                torch.cuda.synchronize()
                out(f"  stored {n_docs:8d} x {ld:3d} tokens, dim {H}: " + ", ".join(f"{f} {n_tok * row[f] / 1e9:.2f} GB ({row[f]} bytes per token)" for f in FORMS) +
                    f"; mxfp4 / int8 = {row['mxfp4'] / row['i8']:.3f}, mxfp4 / f16 = {row['mxfp4'] / row['f16']:.3f}")
                for nq in (1, 8, 64):
                    q = unit(nq * lq)
                    qcu = torch.arange(0, nq + 1, dtype=torch.int32, device=dev) * lq
                    res = {f: (torch.empty(nq, k, dtype=torch.int32, device=dev), torch.empty(nq, k, dtype=torch.float32, device=dev)) for f in FORMS}
                    host = lambda f: (res[f][0].cpu().numpy().copy(), res[f][1].cpu().numpy().copy().view(np.int32))

                    def scan(f, n=nq, at=0):
                        return lambda: index[f].search_device(n, qcu.data_ptr(), q.data_ptr() + at * lq * H * 2, lq, k, res[f][0].data_ptr(), res[f][1].data_ptr(), stream)

                    nc = min(n_cand, n_docs)
                    cand = torch.randint(0, n_docs, (nq, nc), generator=gen, device=dev, dtype=torch.int32)

                    def rescore(f, c=cand, n=nc):
                        return lambda: index[f].rescore_device(nq, qcu.data_ptr(), q.data_ptr(), n, c.data_ptr(), k, res[f][0].data_ptr(), res[f][1].data_ptr(), stream)

                    # the mxfp4 form against itself: the batch, its last query alone, a rescore of the batch's ids
                    scan("mxfp4")(); torch.cuda.synchronize()
                    want = host("mxfp4")
                    ids = res["mxfp4"][0].clone()
                    rescore("mxfp4", ids, k)(); torch.cuda.synchronize()
                    same = all(np.array_equal(x, y) for x, y in zip(host("mxfp4"), want))
                    scan("mxfp4", 1, nq - 1)(); torch.cuda.synchronize()
                    same = same and all(np.array_equal(x[0], y[nq - 1]) for x, y in zip(host("mxfp4"), want))
                    assert same, ("the mxfp4 form disagrees with itself", H, n_docs, nq)

                    def line(what, t, hbm):
                        mx = t["mxfp4"][0]
                        got = {f: res[f][0].cpu().numpy() for f in FORMS}
                        ov = [float(np.mean([len(set(x[x >= 0]) & set(y[y >= 0])) / max(1, int((x >= 0).sum())) for x, y in zip(got["f16"], got[f])])) for f in ("i8", "mxfp4")]
                        r = [t[f][0] / mx for f in ("f16", "i8")]
                        mark = ["**" if x < 1.0 else "  " for x in r]
                        out(f"  {what:36s} {H:5d} {nq:4d} | " + " | ".join(f"{t[f][0]:9.1f} (.. {t[f][1]:.1f})" for f in FORMS) +
                            f" | {mark[0]}{r[0]:5.2f}{mark[0]} | {mark[1]}{r[1]:5.2f}{mark[1]} | {ov[0]:.3f}, {ov[1]:.3f} | {hbm}")

                    t = measure({f: scan(f) for f in FORMS})
                    torch.cuda.synchronize()
                    line(f"scan {n_docs:8d} x {ld:3d} tokens", t, ", ".join(f"{nq * n_tok * row[f] / (t[f][0] * 1e-6) / 1e12 / HBM_TBS:.3f}" for f in FORMS))
                    t = measure({f: rescore(f) for f in FORMS})
                    torch.cuda.synchronize()
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
