#!/usr/bin/env python3
"""Rate of the token index (bert_hip_token_index_search_device / _rescore_device) on one GPU beside two baselines on the same f16 rows:

    (a) what a user could do before the index: bert_hip_maxsim_device on all pairs (a pair list for a rescore) plus torch.topk — as many
        queries per call as keep a launch under 2^32 threads (one workgroup of 256 per pair).  That split is no longer needed: the
        library now cuts a call into launches of at most 2^23 pairs itself (when profiles/token_index_rate.txt was measured, a larger
        all-pairs call returned 0 and left the pairs beyond that unwritten); it stays so that the table's figures keep their meaning
    (b) torch: einsum + amax + sum + topk, the documents in slabs whose intermediate [nq, docs, lq, ld] stays under 2 GiB

    workloads (dim 384, queries of 32 tokens, k = 10; 1, 8 and 64 queries):
      scan     10^5 documents of 180 tokens (13.8 GB of rows) and 10^6 documents of 25 tokens (19.2 GB), generated on the device
      rescore  1000 candidates per query over the same indexes

    python tools/token_index_rate.py [--scale 1.0] [--rounds 3] [--budget-ms 400] [--out profiles/token_index_rate.txt]

Everything is in device memory; a figure is the time per call from device events around back-to-back calls on one stream (as many as
fit --budget-ms, at least 2, after a warm-up call of every implementation), the median of --rounds rounds, the implementations
alternating within each round.  --scale shrinks the document counts (a smoke run).  The scan's line also states the share of the HBM
line, n_tokens dim 2 bytes per QUERY over the time against 8.0 TB/s (the rows are read once per query unless a cache keeps them), and
of the f16 MFMA rate, 2 dim per (query token, document token) against 2517 TFLOP/s, and names the larger share as the bound.  The
index's scores are checked against (a)'s: equal bits."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS, MFMA_TFLOPS = 8.0, 2517.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("token_index_rate.py needs a GPU")
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
        H, lq, k, n_cand = 384, 32, 10, 1000
        unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
        out(f"# token index against (a) bert_hip_maxsim_device + torch.topk and (b) torch einsum + amax + sum + topk, f16 rows, dim {H}, queries of {lq} tokens, "
            f"k = {k}; {torch.cuda.get_device_name(0)}, torch {torch.__version__}; us per call = median (min .. max) of {a.rounds} rounds between device events, "
            f"implementations alternating; scale {a.scale}")
        out("# case                              nq |   index us (min .. max) | (a) maxsim+topk us | (b) torch us | (a) / index | (b) / index | HBM share  MFMA share  bound")
        stream = torch.cuda.current_stream().cuda_stream
        for n_docs, ld in ((int(100000 * a.scale), 180), (int(1000000 * a.scale), 25)):
            n_tok = n_docs * ld
            d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
            for t0 in range(0, n_tok, 1 << 20):
                d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
            dcu_h = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
            dcu = torch.from_numpy(dcu_h).to(dev)
            ix = m.token_index(H)
            ix.reserve(n_docs, n_tok, 64, lq, k)
            assert ix.add_device(dcu_h, d.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            d3 = d.view(n_docs, ld, H)
            for nq in (1, 8, 64):
                q = unit(nq * lq)
                q3 = q.view(nq, lq, H)
                qcu = torch.arange(0, nq + 1, dtype=torch.int32, device=dev) * lq
                ids = torch.empty(nq, k, dtype=torch.int32, device=dev)
                sc = torch.empty(nq, k, dtype=torch.float32, device=dev)
                all_scores = torch.empty(nq, n_docs, dtype=torch.float32, device=dev)
                slab = max(1, (2 << 30) // (nq * lq * ld * 2))
                res = {}

                def index_scan():
                    ix.search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, ids.data_ptr(), sc.data_ptr(), stream)

                qa = max(1, min(nq, (2 ** 32 - 1) // (256 * n_docs)))       # queries per maxsim call, as the table was measured (no longer needed: see above)

                def maxsim_topk():
                    for q0 in range(0, nq, qa):
                        m.maxsim_device(q.data_ptr(), qcu[q0:].data_ptr(), min(qa, nq - q0), d.data_ptr(), dcu.data_ptr(), n_docs, H, None, 0,
                                        all_scores[q0:].data_ptr(), False, stream)
                    res["a"] = torch.topk(all_scores, k, dim=1)

                def torch_topk():
                    parts = [torch.einsum("aih,bjh->abij", q3, d3[b0:b0 + slab]).amax(dim=3).sum(dim=2, dtype=torch.float32) for b0 in range(0, n_docs, slab)]
                    res["b"] = torch.topk(torch.cat(parts, dim=1), k, dim=1)

                t = measure({"index": index_scan, "a": maxsim_topk, "b": torch_topk})
                torch.cuda.synchronize()
                assert torch.equal(sc, res["a"].values), "the scan's scores are not maxsim's"
                us = t["index"][0]
                hbm = nq * n_tok * H * 2 / (us * 1e-6) / 1e12 / HBM_TBS
                mfma = 2.0 * H * nq * lq * n_tok / (us * 1e-6) / 1e12 / MFMA_TFLOPS
                out(f"  scan {n_docs:8d} x {ld:3d} tokens       {nq:4d} | {us:10.1f} ({t['index'][1]:.1f} .. {t['index'][2]:.1f}) | {t['a'][0]:18.1f} | {t['b'][0]:12.1f} | "
                    f"{t['a'][0] / us:11.2f} | {t['b'][0] / us:11.2f} | {hbm:9.3f} {mfma:11.3f}  {'HBM' if hbm > mfma else 'MFMA'}")

                # rescoring 1000 candidates per query
                nc = min(n_cand, n_docs)
                cand = torch.randint(0, n_docs, (nq, nc), generator=gen, device=dev, dtype=torch.int32)
                pairs = torch.stack([torch.arange(nq, device=dev, dtype=torch.int32).repeat_interleave(nc), cand.reshape(-1)], dim=1).contiguous()
                pair_scores = torch.empty(nq * nc, dtype=torch.float32, device=dev)

                def index_rescore():
                    ix.rescore_device(nq, qcu.data_ptr(), q.data_ptr(), nc, cand.data_ptr(), k, ids.data_ptr(), sc.data_ptr(), stream)

                def maxsim_pairs_topk():
                    m.maxsim_device(q.data_ptr(), qcu.data_ptr(), nq, d.data_ptr(), dcu.data_ptr(), n_docs, H, pairs.data_ptr(), nq * nc, pair_scores.data_ptr(), False, stream)
                    res["a"] = torch.topk(pair_scores.view(nq, nc), k, dim=1)

                def torch_gather_topk():
                    g = d3[cand.long()]                                      # [nq, nc, ld, H]
                    res["b"] = torch.topk(torch.einsum("aih,abjh->abij", q3, g).amax(dim=3).sum(dim=2, dtype=torch.float32), k, dim=1)

                t = measure({"index": index_rescore, "a": maxsim_pairs_topk, "b": torch_gather_topk})
                torch.cuda.synchronize()
                assert torch.equal(sc, res["a"].values), "the rescore's scores are not maxsim's"
                us = t["index"][0]
                out(f"  rescore {nc:5d} of {n_docs:8d} x {ld:3d} {nq:4d} | {us:10.1f} ({t['index'][1]:.1f} .. {t['index'][2]:.1f}) | {t['a'][0]:18.1f} | {t['b'][0]:12.1f} | "
                    f"{t['a'][0] / us:11.2f} | {t['b'][0] / us:11.2f} |         -           -  -")
            ix.close()
            del d, d3
            torch.cuda.empty_cache()
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
