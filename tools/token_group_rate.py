#!/usr/bin/env python3
"""Rate of the f16 token index's scan under the tuning key "token_index_query_group" on one GPU, beside torch on the same f16 rows:

    arms      key 1 (the ungrouped kernel: one workgroup per (query, slice)), key 2, key 3, key 4 (the grouped kernel: that many
              consecutive queries a workgroup, every document block read once per group), and torch einsum + amax + sum + topk, the
              documents in slabs whose intermediate [nq, docs, lq, ld] stays under 2 GiB
    workloads 10^6 documents of 25 tokens and 10^5 documents of 180 tokens, at dim 384 and 128, queries of 32 tokens, k = 10,
              1 / 8 / 64 queries

    python tools/token_group_rate.py [--scale 1.0] [--rounds 5] [--budget-ms 250] [--out profiles/token_group_rate.txt]

One process, everything in device memory.  Before anything is timed, ids and score bits of every grouped arm are compared with key 1's.
A figure is the time per call from device events around back-to-back calls on one stream (as many as fit --budget-ms, after a warm-up
call of every arm), the arms interleaved within each round, the FASTEST of --rounds rounds with min .. max beside it.  The last
columns name the fastest key and the G the plan may take from the cell: the fastest grouped arm where it beats key 1 by more than the
cell's spread (the larger of the two arms' max - min), else 1.  --scale shrinks the document counts (a smoke run)."""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = (1, 2, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget-ms", type=float, default=250.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("token_group_rate.py needs a GPU")
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

    def measure(arms):
        """arms: name -> callable; us per call (fastest, min, max) per name, the arms interleaved within each round"""
        iters = {}
        for name, f in arms.items():
            f(); torch.cuda.synchronize()
            iters[name] = int(max(1, min(100, a.budget_ms * 1e3 / max(timed(f, 1), 1.0))))
        t = {name: [] for name in arms}
        for _ in range(a.rounds):
            for name, f in arms.items():
                t[name].append(timed(f, iters[name]))
        return {name: (min(v), min(v), max(v)) for name, v in t.items()}

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)        # (a context to launch from: the kernels do not read the model)
        m = pybert.BertModel(path)
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(1)
        lq, k = 32, 10
        out(f"# f16 token index scan under \"token_index_query_group\" 1 (ungrouped) / 2 / 3 / 4 and torch einsum + amax + sum + topk, queries of {lq} tokens, "
            f"k = {k}; {torch.cuda.get_device_name(0)}, torch {torch.__version__}; us per call = fastest (min .. max) of {a.rounds} rounds between device events, "
            f"arms interleaved; ids and score bits of keys 2 / 3 / 4 equal key 1's in every cell (checked before timing); scale {a.scale}")
        out("# dim  documents x tokens   nq |  key 1 us (min .. max) |  key 2 us (min .. max) |  key 3 us (min .. max) |  key 4 us (min .. max) |  torch us (min .. max) |"
            " best key / key 1 | torch / key 1 | torch / best | planned G")
        stream = torch.cuda.current_stream().cuda_stream
        for H in (384, 128):
            unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
            for n_docs, ld in ((int(1000000 * a.scale), 25), (int(100000 * a.scale), 180)):
                n_tok = n_docs * ld
                d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
                for t0 in range(0, n_tok, 1 << 20):
                    d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
                dcu_h = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
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
                    slab = max(1, (2 << 30) // (nq * lq * ld * 2))

                    def scan(key):
                        def f():
                            m.set_option("token_index_query_group", str(key))
                            ix.search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, ids.data_ptr(), sc.data_ptr(), stream)
                        return f

                    def torch_topk():
                        parts = [torch.einsum("aih,bjh->abij", q3, d3[b0:b0 + slab]).amax(dim=3).sum(dim=2, dtype=torch.float32) for b0 in range(0, n_docs, slab)]
                        return torch.topk(torch.cat(parts, dim=1), k, dim=1)

                    # ids and score bits of every grouped arm against key 1, before anything is timed
                    scan(1)(); torch.cuda.synchronize()
                    ref = ids.clone(), sc.clone()
                    for key in KEYS[1:]:
                        ids.fill_(-7); sc.fill_(float("nan"))
                        scan(key)(); torch.cuda.synchronize()
                        assert torch.equal(ids, ref[0]) and torch.equal(sc.view(torch.int32), ref[1].view(torch.int32)), (H, n_docs, nq, key)
                    arms = {f"key {key}": scan(key) for key in KEYS}
                    arms["torch"] = torch_topk
                    t = measure(arms)
                    torch.cuda.synchronize()
                    one = t["key 1"]
                    best = min(KEYS, key=lambda key: t[f"key {key}"][0])
                    tb = t[f"key {best}"]
                    spread = max(one[2] - one[1], tb[2] - tb[1])
                    planned = best if best > 1 and one[0] - tb[0] > spread else 1
                    cells = " | ".join(f"{t[name][0]:9.1f} ({t[name][1]:.1f} .. {t[name][2]:.1f})" for name in arms)
                    out(f"  {H:4d} {n_docs:8d} x {ld:3d}      {nq:4d} | {cells} | key {best} {tb[0] / one[0]:9.2f} | {t['torch'][0] / one[0]:13.2f} | "
                        f"{t['torch'][0] / tb[0]:12.2f} | {planned}")
                m.set_option("token_index_query_group", "0")
                ix.close()
                del d, d3
                torch.cuda.empty_cache()
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
