#!/usr/bin/env python3
"""Rate of the sparse index's search (bert_hip_sparse_index_search_device) on one GPU: 10^6 synthetic rows of up to 128 terms drawn
Zipf-like over V = 30 522, queries of up to 32 terms drawn the same way, both dtypes, 1 / 64 / 4096 queries, k = 10 and 100.

    python tools/sparse_index_rate.py [--rows 1000000] [--qb 1,2,4,8] [--sections search,filtered,rescore,inverted] [--out profiles/sparse_index_rate.txt] [--append]

Per cell: the time per call (device events around back-to-back calls on one stream, the median of the rounds); the bytes of stored terms
the call reads (every query tile walks every row's terms once: ids + weights of the stored terms, 8 or 4 bytes each, times the tiles) over
that time, as a share of the project's HBM line (4.8 TB/s) — a share above 1 means the tiles of a slice found it in L2 —;
and the same search by torch: a sparse_csr_tensor [rows, V] of the stored weights times the dense queries [V, nq], then topk — where this
torch build can run it (the script says so where it cannot).  --qb: the A/B of the scan's tile size (queries per workgroup, the tuning
key "sparse_index_qb") at 64 and 4096 queries, which sparse_index_kernels.h's SPARSE_QB was chosen from.
--sections: "search" is the table above (the default); "filtered": search_filtered_device at k = 10 with 1 and 64 queries under
allow-lists of 100 %, 50 % and 1 % of the rows at random and 1 % in contiguous 64-row blocks, beside the plain search, and the plain
search again on an index whose rows were removed down to the same 50 % (the masked scan through the live bits); "rescore":
rescore_device of 1000 candidates per query (distinct random rows) beside a filtered search of one query under an allow-list of exactly
such candidates; "inverted": search_inverted_device beside search_device on the same index in the same process, the runs interleaved
(one timed run of each per repeat, min .. max of --repeats repeats), at 1 / 64 / 4096 queries and k = 10 and 100, with the time of
invert and the postings' bytes, on two row distributions — ids = V u^3 (the workload above: some terms are in most rows) and uniformly
random ids (which flatters an inverted search: every list is short) —, a sweep of the tuning key "sparse_index_segment_rows" over
--segments at 1, 64 and 4096 queries and the tile size's A/B ("sparse_index_qb" 1 and 4 against the plan's 2; the key is the row-major scan's too) at the default segment size, and per cell the floor of the arithmetic: the postings of the queries' lists read once at the HBM
line plus one pass over 4 bytes per (row, query) of LDS accumulators at the LDS line.  Both searches' results are compared, ids and
score bits, before anything is timed.  --append adds to --out instead of replacing it.
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
    ap.add_argument("--sections", default="search")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--segments", default="512,1024,2048,4096,8192,16384")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sections = set(a.sections.split(","))
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

    def terms(n, kk, power=3):
        """ids [n, kk] i32 (Zipf-like: V u^3; a repeat within a row becomes -1) and weights [n, kk] f32 in (0, 2)"""
        ids = (V * torch.rand(n, kk, device=dev, generator=gen) ** power).to(torch.int32).clamp_(max=V - 1)
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
        LDS_LINE = 256 * 128 * 2.4e9                             # bytes/s: 4-byte LDS reads at 128 bytes a clock and CU, 256 CUs, 2.4 GHz
        uniform = (terms(N, W, 1), terms(4096, KQ, 1)) if "inverted" in sections else None

        def pair_timed(f_inv, f_row):
            """(min, max) ms of each over --repeats repeats; a repeat times one run of back-to-back calls of each, interleaved"""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = ([], [])
            iters = []
            for f in (f_inv, f_row):
                f()
                torch.cuda.synchronize()
                e0.record(); f(); e1.record(); e1.synchronize()
                iters.append(int(max(1, min(50, 100.0 / max(e0.elapsed_time(e1), 1e-3)))))
            for _ in range(a.repeats):
                for f, it, t in zip((f_inv, f_row), iters, ts):
                    e0.record()
                    for _ in range(it):
                        f()
                    e1.record()
                    e1.synchronize()
                    t.append(e0.elapsed_time(e1) / it)
            return (min(ts[0]), max(ts[0])), (min(ts[1]), max(ts[1]))

        def inverted_section(dtype, ix_readme, d_ids, d_sc):
            import time
            wb = idb = 4 if dtype == "f32" else 2
            d_ids2, d_sc2 = torch.empty_like(d_ids), torch.empty_like(d_sc)
            for dist, rows_q in (("ids = V u^3", None), ("uniform ids", uniform)):
                if rows_q is None:
                    ixd, rid, qi, qw = ix_readme, r_ids, q_ids, q_w
                else:
                    (rid, rw), (qi, qw) = rows_q
                    ixd = m.sparse_index(W, dtype, n_vocab=V)
                    ixd.reserve(N, 4096, 100)
                    for r0 in range(0, N, 100000):
                        c = min(100000, N - r0)
                        ixd.add_device(c, W, rid[r0:r0 + c].data_ptr(), rw[r0:r0 + c].data_ptr(), stream)
                    torch.cuda.synchronize()
                # the rows that hold each id: the length of its posting list over the whole index
                df = torch.bincount(rid[rid >= 0].long(), minlength=V)
                nt = int((rid >= 0).sum())

                def inv(nq, k):
                    ixd.search_inverted_device(nq, KQ, qi.data_ptr(), qw.data_ptr(), k, d_ids2.data_ptr(), d_sc2.data_ptr(), stream)

                def rowm(nq, k):
                    ixd.search_device(nq, KQ, qi.data_ptr(), qw.data_ptr(), k, d_ids.data_ptr(), d_sc.data_ptr(), stream)

                def table(seg_label, cells):
                    for nq, k in cells:
                        inv(nq, k); rowm(nq, k)
                        torch.cuda.synchronize()
                        n = nq * k
                        assert torch.equal(d_ids.view(-1)[:n], d_ids2.view(-1)[:n]) and torch.equal(d_sc.view(-1)[:n].view(torch.int32), d_sc2.view(-1)[:n].view(torch.int32)), (dist, nq, k)
                        (ilo, ihi), (rlo, rhi) = pair_timed(lambda: inv(nq, k), lambda: rowm(nq, k))
                        posts = int(df[qi[:nq][qi[:nq] >= 0].long()].sum())
                        floor = posts * (2 + wb) / HBM_LINE * 1e3 + nq * N * 4 / LDS_LINE * 1e3
                        slow = "**" if ilo > rhi else ""
                        out(f"  {seg_label:>6} {nq:5d} {k:4d}   {slow}{ilo:9.3f} .. {ihi:9.3f}{slow}   {rlo:9.3f} .. {rhi:9.3f}   {rlo / ilo:7.2f}   {posts:12d} {floor:9.4f} {ilo / floor:8.1f}")

                out(f"# dtype {dtype}, {dist}: search_inverted_device beside search_device, ms per call, min .. max of {a.repeats} interleaved repeats; "
                    f"** = the inverted search is slower (its fastest repeat against the row-major search's slowest)")
                out("#    seg    nq    k        inverted (min .. max)     row-major (min .. max)   row/inv   postings read  floor ms  inv/floor")
                segs = [int(x) for x in a.segments.split(",")] if rows_q is None else []
                for seg in [0] + segs:
                    m.set_option("sparse_index_segment_rows", str(seg))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert ixd.invert() == N
                    t_inv = (time.perf_counter() - t0) * 1e3
                    sg = seg or 2048
                    n_seg = -(-N // sg)
                    pbytes = n_seg * sg * W * (2 + wb) + n_seg * (V + 1) * 4
                    out(f"#   segment rows {sg}{' (the default)' if not seg else ''}: invert {t_inv:.1f} ms (blocking, with its allocations); postings {pbytes / 1e9:.3f} GB "
                        f"({n_seg * (V + 1) * 4 / 1e6:.1f} MB of them offsets) for {nt * (idb + wb) / 1e9:.3f} GB of stored terms in {-(-N // 64) * 64 * W * (idb + wb) / 1e9:.3f} GB of blocks")
                    table(str(sg), [(nq, k) for nq in (1, 64, 4096) for k in (10, 100)] if not seg else [(1, 10), (64, 10), (4096, 10)])
                m.set_option("sparse_index_segment_rows", "0")
                if rows_q is None:
                    # the tile's A/B at the default segment size (a tile of qb queries keeps qb of the workgroup's four waves walking)
                    assert ixd.invert() == N
                    for qb in (1, 4):
                        m.set_option("sparse_index_qb", str(qb))
                        table(f"qb {qb}", [(64, 10), (4096, 10)])
                    m.set_option("sparse_index_qb", "0")
                if rows_q is not None:
                    ixd.close()

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

            def words_of(mask):
                """a bool [N] device mask as the allow-list's uint32 words (bit b of word w = row 32 w + b), on the device"""
                pad = torch.zeros((N + 31) // 32 * 32, dtype=torch.int64, device=dev)
                pad[:N] = mask.to(torch.int64)
                w = (pad.view(-1, 32) << torch.arange(32, device=dev, dtype=torch.int64)).sum(dim=1)
                return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()      # (the words' bits as i32)

            def cell(label, f, note=""):
                ms, lo, hi = timed(f)
                out(f"  {label:58s} {ms:9.3f} ({lo:.3f} .. {hi:.3f})   {note}")
                return ms

            if "filtered" in sections:
                out(f"# dtype {dtype}: search_filtered_device, k = 10; blocks = the share of 64-row blocks with an allowed row; x = time / the plain search's")
                blocks = N // 64
                masks = {"100 %": torch.ones(N, dtype=torch.bool, device=dev),
                         "50 % random": torch.rand(N, device=dev, generator=gen) < 0.5,
                         "1 % random": torch.rand(N, device=dev, generator=gen) < 0.01}
                clustered = torch.zeros(N, dtype=torch.bool, device=dev)
                pick = torch.randperm(blocks, device=dev, generator=gen)[:max(1, blocks // 100)]
                clustered.view(-1)[:blocks * 64].view(blocks, 64)[pick] = True
                masks["1 % in contiguous blocks"] = clustered
                for nq in (1, 64):
                    base = cell(f"nq {nq:2d}  plain search (the unmasked kernel)", lambda: search(nq, 10))
                    for name, mask in masks.items():
                        d_allow = words_of(mask)
                        share = float(mask[:blocks * 64].view(blocks, 64).any(dim=1).float().mean())
                        ms = cell(f"nq {nq:2d}  allow {name} ({int(mask.sum())} rows)",
                                  lambda: ix.search_device(nq, KQ, q_ids.data_ptr(), q_w.data_ptr(), 10, d_ids.data_ptr(), d_sc.data_ptr(), stream,
                                                           d_allow.data_ptr(), d_allow.numel()))
                        lines[-1] += f"blocks {share:.3f}  x {ms / base:.2f}"
                        print(f"      blocks {share:.3f}  x {ms / base:.2f}", flush=True)
                        torch.cuda.synchronize()
                        del d_allow

            if "rescore" in sections:
                out(f"# dtype {dtype}: rescore_device of 1000 candidates a query, k = 10, beside one filtered query under an allow-list of 1000 such rows")
                n_cand = 1000
                cand = torch.stack([torch.randperm(N, device=dev, generator=gen)[:n_cand] for _ in range(64)]).to(torch.int32).contiguous()
                for nq in (1, 64):
                    cell(f"nq {nq:2d}  rescore_device, n_cand {n_cand}",
                         lambda: ix.rescore_device(nq, KQ, q_ids.data_ptr(), q_w.data_ptr(), n_cand, cand.data_ptr(), 10, d_ids.data_ptr(), d_sc.data_ptr(), stream))
                one = torch.zeros(N, dtype=torch.bool, device=dev)
                one[cand[0].long()] = True
                d_allow = words_of(one)
                # the two agree on the first query: the same ids and score bits
                ix.rescore_device(1, KQ, q_ids.data_ptr(), q_w.data_ptr(), n_cand, cand.data_ptr(), 10, d_ids.data_ptr(), d_sc.data_ptr(), stream)
                torch.cuda.synchronize()
                r_i, r_s = d_ids.view(-1)[:10].clone(), d_sc.view(-1)[:10].clone()
                cell("nq  1  search_filtered_device, the same 1000 rows allowed",
                     lambda: ix.search_device(1, KQ, q_ids.data_ptr(), q_w.data_ptr(), 10, d_ids.data_ptr(), d_sc.data_ptr(), stream, d_allow.data_ptr(), d_allow.numel()))
                torch.cuda.synchronize()
                assert torch.equal(r_i, d_ids.view(-1)[:10]) and torch.equal(r_s.view(torch.int32), d_sc.view(-1)[:10].view(torch.int32))

            def removals():
                """the masked scan through the live bits.  Last of all: the index is not the same afterwards"""
                if "filtered" not in sections:
                    return
                half = torch.nonzero(~masks["50 % random"]).view(-1).to(torch.int32).cpu().numpy()
                ix.remove(half)
                for nq in (1, 64):
                    cell(f"nq {nq:2d}  plain search after removing {len(half)} rows (masked kernel)", lambda: search(nq, 10))

            if "inverted" in sections:
                inverted_section(dtype, ix, d_ids, d_sc)

            m_qb = None
            if "search" in sections:
                out(f"# dtype {dtype}: search_device")
                out("#   nq    k   qb tiles slices        ms (min .. max)      queries/s   GB read    share   torch csr @ dense + topk")
            for nq in (1, 64, 4096) if "search" in sections else ():
                for k in (10, 100):
                    row(nq, k, with_torch=True)
            # the tile size's A/B
            if a.qb and "search" in sections:
                out(f"# dtype {dtype}: tile size A/B (set_option sparse_index_qb), k = 10")
                for nq in (64, 4096):
                    for qb in a.qb.split(","):
                        m.set_option("sparse_index_qb", qb)
                        m_qb = qb
                        row(nq, 10, with_torch=False)
                m.set_option("sparse_index_qb", "0")
                m_qb = None
            # a sanity check of the last result: ids in range, scores descending
            if "search" not in sections:
                removals()
                ix.close()
                continue
            search(64, 10)
            torch.cuda.synchronize()
            got_i, got_s = d_ids[:64 * 10].view(-1)[:640].view(64, 10), d_sc.view(-1)[:640].view(64, 10)
            assert bool(((got_i >= 0) & (got_i < N)).all()) and bool((got_s[:, 1:] <= got_s[:, :-1]).all())
            removals()
            ix.close()
            csr = None
        m.close()
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
