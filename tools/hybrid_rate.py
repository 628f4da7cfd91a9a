#!/usr/bin/env python3
"""Cost of a hybrid search (bert_hip_hybrid_search_device) on one GPU beside the two searches it is made of: the workload of
tools/sparse_index_rate.py — 10^6 synthetic rows of up to 128 terms drawn Zipf-like over V = 30 522, queries of up to 32 terms, k = 10 —
and a dense index of the same 10^6 rows beside it, dim 384, unit rows.  Dense dtypes f16 and i8, sparse dtypes f32 and f16, 1 / 64 / 4096
queries.

    python tools/hybrid_rate.py [--rows 1000000] [--chunks 32,64,256] [--out profiles/hybrid_rate.txt]

Per cell, in one run: the time per call of hybrid_search_device, of bert_hip_index_search_device and of
bert_hip_sparse_index_search_device on the same indexes (device events around back-to-back calls on one stream, the median of the
rounds, the three measured in turn within each round), the hybrid call over the sum of the two, the time one write and one read of the
score matrix take at the project's HBM line (8 bytes x queries x rows over 4.8 TB/s), and — from a second, profiled
call, never the timed one — the per-kernel split of the hybrid call by the engine's profiler.  --chunks: the A/B of the tuning key
"hybrid_chunk_queries" at 4096 queries.  Everything is in device memory; the rows are generated on the device.

    python tools/hybrid_rate.py --section inverted [--out profiles/hybrid_inverted_rate.txt]

The hybrid search over the postings (bert_hip_dense_sparse_search_inverted_device) beside bert_hip_hybrid_search_device on the same
indexes in the same process: per cell both calls' ids and score bits are compared, then the two are timed in turn, the fastest of five
rounds and the slowest beside it; the per-kernel split of both for the f16 x f32 cells; the time of invert, once per sparse index.
The load-placement A/B of DESIGN.md §15.1 is this section under two libraries built by tools/variant.sh
(-DSPARSE_POSTINGS_D_AHEAD=1 and =0), chosen by BERT_HIP_LIB, in one job."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_LINE = 4.8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--kq", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunks", default="32,64,256")
    ap.add_argument("--dense", default="f16,i8")
    ap.add_argument("--sparse", default="f32,f16")
    ap.add_argument("--queries", default="1,64,4096")
    ap.add_argument("--out", default=None)
    ap.add_argument("--section", default="hybrid", choices=["hybrid", "inverted"],
                    help="inverted: bert_hip_dense_sparse_search_inverted_device beside bert_hip_hybrid_search_device, cell by cell")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hybrid_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    V, N, W, KQ, DIM, K = 30522, a.rows, a.width, a.kq, a.dim, a.k
    NQ = [int(x) for x in a.queries.split(",")]
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def terms(n, kk):
        """ids [n, kk] i32 (Zipf-like: V u^3; a repeat within a row becomes -1) and weights [n, kk] f32 in (0, 2): sparse_index_rate.py's"""
        ids = (V * torch.rand(n, kk, device=dev, generator=gen) ** 3).to(torch.int32).clamp_(max=V - 1)
        ids, _ = torch.sort(ids, dim=1)
        ids[:, 1:][ids[:, 1:] == ids[:, :-1]] = -1
        w = torch.rand(n, kk, device=dev, generator=gen) * 2 + 1e-3
        return ids.contiguous(), w.contiguous()

    def unit(n):
        x = torch.randn(n, DIM, device=dev, generator=gen)
        return (x / x.norm(dim=1, keepdim=True)).contiguous()

    def timed_in_turn(fs, budget_ms=400.0, max_iters=50):
        """the calls of fs measured in turn within each round: per call (median, min, max) ms"""
        iters = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for f in fs:
            f()
            torch.cuda.synchronize()
            e0.record(); f(); e1.record(); e1.synchronize()
            iters.append(int(max(1, min(max_iters, budget_ms / max(e0.elapsed_time(e1), 1e-3)))))
        ts = [[] for _ in fs]
        for _ in range(a.rounds):
            for i, f in enumerate(fs):
                e0.record()
                for _ in range(iters[i]):
                    f()
                e1.record()
                e1.synchronize()
                ts[i].append(e0.elapsed_time(e1) / iters[i])
        return [(float(np.median(t)), min(t), max(t)) for t in ts]

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)          # (any model: the indexes only need the context's device)
        m = pybert.BertModel(path)
        r_ids, r_w = terms(N, W)
        q_ids, q_w = terms(max(NQ), KQ)
        q = unit(max(NQ))
        out(f"# bert_hip_hybrid_search_device, {torch.cuda.get_device_name(0)}: {N} rows; dense dim {DIM}, unit rows; sparse width {W} "
            f"({float((r_ids >= 0).sum()) / N:.1f} terms a row, ids = V u^3 over V = {V}), queries of {KQ} columns; k = {K}; weights 0.5, 0.5")
        out(f"# ms per call = median (min .. max) of {a.rounds} rounds of back-to-back calls between device events, the three calls of a cell in turn "
            "within each round; matrix = 8 bytes x queries x rows / 4.8 TB/s, one write and one read of the dense scores")
        dense, sparse = {}, {}
        for dd in a.dense.split(","):
            dense[dd] = m.index(DIM, dd)
        for sd in a.sparse.split(","):
            sparse[sd] = m.sparse_index(W, sd, n_vocab=V)
        gen.manual_seed(2)
        for r0 in range(0, N, 100000):
            c = min(100000, N - r0)
            rows = unit(c)
            for ix in dense.values():
                ix.add_device(c, rows.data_ptr(), stream)
            for ix in sparse.values():
                ix.add_device(c, W, r_ids[r0:r0 + c].data_ptr(), r_w[r0:r0 + c].data_ptr(), stream)
            torch.cuda.synchronize()
        d_ids = torch.empty(max(NQ), K, dtype=torch.int32, device=dev)
        d_sc = torch.empty(max(NQ), K, dtype=torch.float32, device=dev)

        def split(f):
            """the engine's per-kernel times of one call of f: name -> (launches, ms)"""
            torch.cuda.synchronize()
            m.profile(True)
            m.profile_report()                                   # (clears what was collected)
            f()
            torch.cuda.synchronize()
            rep = m.profile_report()
            m.profile(False)
            return {name: (v["launches"], v["total_ms"]) for name, v in rep.items() if isinstance(v, dict) and v.get("launches")}

        def fastest_in_turn(fs, rounds=5, budget_ms=300.0, max_iters=50):
            """the calls of fs interleaved, `rounds` rounds: per call (fastest, slowest) ms of a round's mean"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            iters = []
            for f in fs:
                f()
                torch.cuda.synchronize()
                e0.record(); f(); e1.record(); e1.synchronize()
                iters.append(int(max(1, min(max_iters, budget_ms / max(e0.elapsed_time(e1), 1e-3)))))
            ts = [[] for _ in fs]
            for _ in range(rounds):
                for i, f in enumerate(fs):
                    e0.record()
                    for _ in range(iters[i]):
                        f()
                    e1.record()
                    e1.synchronize()
                    ts[i].append(e0.elapsed_time(e1) / iters[i])
            return [(min(t), max(t)) for t in ts]

        if a.section == "inverted":
            # the hybrid search over the postings beside the one over the rows: the same indexes, the same process, the runs interleaved
            import time
            out("# section inverted: bert_hip_dense_sparse_search_inverted_device (new) beside bert_hip_hybrid_search_device (rows), the same "
                "indexes and queries; ms per call = the fastest of 5 interleaved rounds (slowest in brackets); ids and score bits of the two "
                "calls compared in every cell before it is timed")
            for sd, six in sparse.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                six.invert()
                torch.cuda.synchronize()
                out(f"# sparse {sd}: bert_hip_sparse_index_invert of {N} rows, once: {(time.perf_counter() - t0) * 1e3:.1f} ms (blocking, wall clock)")
            a_i, a_s = torch.empty_like(d_ids), torch.empty_like(d_sc)
            for dd, dix in dense.items():
                for sd, six in sparse.items():
                    dix.hybrid_reserve(six, N, max(NQ), K)
                    out(f"# dense {dd} x sparse {sd}")
                    out("#   nq    HC     rows ms (slowest)    postings ms (slowest)   postings/rows   bits")
                    for nq in NQ:
                        hc = pybert.test_hybrid_chunk(N, nq, 0)[0]
                        rows_call = lambda: dix.hybrid_search_device(six, nq, q.data_ptr(), KQ, q_ids.data_ptr(), q_w.data_ptr(), K, d_ids.data_ptr(), d_sc.data_ptr(), 0.5, 0.5, stream)
                        post_call = lambda: dix.hybrid_search_inverted_device(six, nq, q.data_ptr(), KQ, q_ids.data_ptr(), q_w.data_ptr(), K, a_i.data_ptr(), a_s.data_ptr(), 0.5, 0.5, stream)
                        rows_call(); post_call()
                        torch.cuda.synchronize()
                        equal = bool((d_ids[:nq] == a_i[:nq]).all()) and bool((d_sc[:nq].view(torch.int32) == a_s[:nq].view(torch.int32)).all())
                        (r, rhi), (p, phi) = fastest_in_turn([rows_call, post_call])
                        out(f"  {nq:5d} {hc:5d} {r:10.3f} ({rhi:.3f}) {p:14.3f} ({phi:.3f}) {p / r:15.3f}   {'equal' if equal else 'DIFFERENT'}")
                        if (dd, sd) == ("f16", "f32"):
                            for tag, f in (("rows", rows_call), ("postings", post_call)):
                                sp = split(f)
                                out(f"#         {tag:8s} split: " + ", ".join(f"{name} {n} x {ms / n:.3f}" for name, (n, ms) in sorted(sp.items(), key=lambda kv: -kv[1][1])))
                        assert equal, (dd, sd, nq)
            dense.clear()

        for dd, dix in dense.items():
            for sd, six in sparse.items():
                dix.hybrid_reserve(six, N, max(NQ), K)
                out(f"# dense {dd} x sparse {sd}")
                out("#   nq    HC       hybrid ms (min .. max)        dense ms        sparse ms       sum   hybrid/sum   hybrid-sum   matrix ms   per-kernel split of the hybrid call (launches x ms)")

                def calls(nq):
                    return [lambda: dix.hybrid_search_device(six, nq, q.data_ptr(), KQ, q_ids.data_ptr(), q_w.data_ptr(), K, d_ids.data_ptr(), d_sc.data_ptr(), 0.5, 0.5, stream),
                            lambda: dix.search_device(nq, q.data_ptr(), K, d_ids.data_ptr(), d_sc.data_ptr(), stream),
                            lambda: six.search_device(nq, KQ, q_ids.data_ptr(), q_w.data_ptr(), K, d_ids.data_ptr(), d_sc.data_ptr(), stream)]

                def row(nq, pref=0):
                    hc = pybert.test_hybrid_chunk(N, nq, pref)[0]
                    fs = calls(nq)
                    (h, hlo, hhi), (d, _, _), (s, _, _) = timed_in_turn(fs)
                    sp = split(fs[0])
                    txt = ", ".join(f"{name} {n} x {ms / n:.3f}" for name, (n, ms) in sorted(sp.items(), key=lambda kv: -kv[1][1]))
                    matrix = 8.0 * nq * N / HBM_LINE * 1e3
                    out(f"  {nq:5d} {hc:5d} {h:9.3f} ({hlo:.3f} .. {hhi:.3f}) {d:14.3f} {s:16.3f} {d + s:9.3f} {h / (d + s):12.3f} {h - d - s:12.3f} {matrix:11.3f}   {txt}")

                for nq in NQ:
                    row(nq)
                if a.chunks and max(NQ) >= 4096:
                    out(f"# dense {dd} x sparse {sd}: chunk size A/B (set_option hybrid_chunk_queries), 4096 queries")
                    for hc in a.chunks.split(","):
                        m.set_option("hybrid_chunk_queries", hc)
                        row(4096, int(hc))
                    m.set_option("hybrid_chunk_queries", "0")
                # a sanity check of the last result: ids in range, scores descending
                calls(64)[0]()
                torch.cuda.synchronize()
                got_i, got_s = d_ids[:64], d_sc[:64]
                assert bool(((got_i >= 0) & (got_i < N)).all()) and bool((got_s[:, 1:] <= got_s[:, :-1]).all())
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
