#!/usr/bin/env python3
"""Rate of the sparse index's search (bert_hip_sparse_index_search_device) on one GPU: 10^6 synthetic rows of up to 128 terms drawn
Zipf-like over V = 30 522, queries of up to 32 terms drawn the same way, both dtypes, 1 / 64 / 4096 queries, k = 10 and 100.

    python tools/sparse_index_rate.py [--rows 1000000] [--qb 1,2,4,8] [--out profiles/sparse_index_rate.txt]

Per cell: the time per call (device events around back-to-back calls on one stream, the median of the rounds); the bytes of stored terms
the call reads (every query tile walks every row's terms once: ids + weights of the stored terms, 8 or 4 bytes each, times the tiles) over
that time, as a share of the project's HBM line (4.8 TB/s) — a share above 1 means the tiles of a slice found it in L2 —;
and the same search by torch: a sparse_csr_tensor [rows, V] of the stored weights times the dense queries [V, nq], then topk — where this
torch build can run it (the script says so where it cannot).  --qb: the A/B of the scan's tile size (queries per workgroup, the tuning
key "sparse_index_qb") at 64 and 4096 queries, which sparse_index_kernels.h's SPARSE_QB was chosen from.
Everything is in device memory; the rows are generated on the device and added with add_device."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_LINE = 4.8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--kq", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--qb", default="1,2,4,8")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_index_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    V, N, W, KQ = 30522, a.rows, a.width, a.kq
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    def terms(n, kk):
        """ids [n, kk] i32 (Zipf-like: V u^3; a repeat within a row becomes -1) and weights [n, kk] f32 in (0, 2)"""
        ids = (V * torch.rand(n, kk, device=dev, generator=gen) ** 3).to(torch.int32).clamp_(max=V - 1)
        ids, _ = torch.sort(ids, dim=1)
        ids[:, 1:][ids[:, 1:] == ids[:, :-1]] = -1
        w = torch.rand(n, kk, device=dev, generator=gen) * 2 + 1e-3
        return ids.contiguous(), w.contiguous()

    def timed(f, budget_ms=400.0, max_iters=50):
        f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        iters = int(max(1, min(max_iters, budget_ms / max(e0.elapsed_time(e1), 1e-3))))
        ts = []
        for _ in range(a.rounds):
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / iters)
        return float(np.median(ts)), min(ts), max(ts)

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)          # (any model: the index only needs the context's device)
        m = pybert.BertModel(path)
        r_ids, r_w = terms(N, W)
        n_terms = int((r_ids >= 0).sum())
        q_ids, q_w = terms(4096, KQ)
        out(f"# bert_hip_sparse_index_search_device, {torch.cuda.get_device_name(0)}: {N} rows of width {W} ({n_terms / N:.1f} terms a row after dropping "
            f"repeats, ids = V u^3 over V = {V}), queries of {KQ} columns ({float((q_ids >= 0).sum()) / 4096:.1f} terms); ms per call = median "
            f"(min .. max) of {a.rounds} rounds of back-to-back calls between device events")
        out(f"# share = bytes of stored terms read (terms x 8 or 4 bytes x query tiles) / time / {HBM_LINE / 1e12:.1f} TB/s")
        csr = None
        for dtype in ("f32", "f16"):
            code = 0 if dtype == "f32" else 1
            ix = m.sparse_index(W, dtype, n_vocab=V)
            ix.reserve(N, 4096, 100)
            for r0 in range(0, N, 100000):
                c = min(100000, N - r0)
                ix.add_device(c, W, r_ids[r0:r0 + c].data_ptr(), r_w[r0:r0 + c].data_ptr(), stream)
            torch.cuda.synchronize()
            assert len(ix) == N
            term_bytes = n_terms * (8 if dtype == "f32" else 4)
            out(f"# dtype {dtype}: {term_bytes / 1e9:.3f} GB of stored terms")
            out("#   nq    k   qb tiles slices        ms (min .. max)      queries/s   GB read    share   torch csr @ dense + topk")
            d_ids = torch.empty(4096, 100, dtype=torch.int32, device=dev)
            d_sc = torch.empty(4096, 100, dtype=torch.float32, device=dev)

            def search(nq, k):
                ix.search_device(nq, KQ, q_ids.data_ptr(), q_w.data_ptr(), k, d_ids.data_ptr(), d_sc.data_ptr(), stream)

            def row(nq, k, with_torch):
                g = pybert.test_sparse_scan_geometry(code, V, N, nq, k)
                qb = int(m_qb) if m_qb else g["qb"]
                tiles = -(-nq // min(qb, nq))
                ms, lo, hi = timed(lambda: search(nq, k))
                gb = term_bytes * tiles / 1e9
                t = ""
                if with_torch:
                    t = torch_cell(nq, k)
                out(f"  {nq:5d} {k:4d} {min(qb, nq):4d} {tiles:5d} {g['n_slices'] if not m_qb else '-':>6} {ms:9.3f} ({lo:.3f} .. {hi:.3f}) {nq / ms * 1e3:12.0f} {gb:9.2f} "
                    f"{gb * 1e9 / (ms * 1e-3) / HBM_LINE:8.3f}   {t}")
                return ms

            def torch_cell(nq, k):
                nonlocal csr
                if a.no_torch:
                    return "not run (--no-torch)"
                try:
                    if csr is None or csr[0] != dtype:
                        st_i, st_w = ix_rows()
                        counts = (st_i >= 0).sum(dim=1)
                        crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
                        crow[1:] = torch.cumsum(counts, 0)
                        keep = st_i >= 0
                        csr = (dtype, torch.sparse_csr_tensor(crow, st_i[keep].to(torch.int64), st_w[keep], size=(N, V), device=dev))
                    dense = torch.zeros(V, nq, device=dev)
                    qi, qw = q_ids[:nq], q_w[:nq]
                    ok = qi >= 0
                    cols = torch.arange(nq, device=dev).unsqueeze(1).expand_as(qi)
                    dense[qi[ok].long(), cols[ok]] = qw[ok]

                    def f():
                        return torch.topk((csr[1] @ dense).T, k, dim=1)

                    ms, lo, hi = timed(f, budget_ms=200.0, max_iters=10)
                    return f"{ms:9.3f} ms ({lo:.3f} .. {hi:.3f})"
                except Exception as e:                           # (this torch build cannot run it: say so)
                    return f"torch cannot run it here: {type(e).__name__}: {str(e).splitlines()[0][:90]}"

            def ix_rows():
                """the stored rows as device tensors (what torch multiplies): the generated ones, the weights as stored"""
                w = r_w if dtype == "f32" else r_w.half().float()
                return r_ids, w

            m_qb = None
            for nq in (1, 64, 4096):
                for k in (10, 100):
                    row(nq, k, with_torch=True)
            # the tile size's A/B
            if a.qb:
                out(f"# dtype {dtype}: tile size A/B (set_option sparse_index_qb), k = 10")
                for nq in (64, 4096):
                    for qb in a.qb.split(","):
                        m.set_option("sparse_index_qb", qb)
                        m_qb = qb
                        row(nq, 10, with_torch=False)
                m.set_option("sparse_index_qb", "0")
                m_qb = None
            # a sanity check of the last result: ids in range, scores descending
            search(64, 10)
            torch.cuda.synchronize()
            got_i, got_s = d_ids[:64 * 10].view(-1)[:640].view(64, 10), d_sc.view(-1)[:640].view(64, 10)
            assert bool(((got_i >= 0) & (got_i < N)).all()) and bool((got_s[:, 1:] <= got_s[:, :-1]).all())
            ix.close()
            csr = None
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
