#!/usr/bin/env python3
"""What the token index's life cycle costs (bert_hip_late_index_*), on one GPU, with the method of tools/token_index_rate.py: dim 384,
queries of 32 tokens, k = 10, everything in device memory, time per call from device events around back-to-back calls on one stream (as
many as fit --budget-ms, at least 2, after a warm-up call of every implementation), the median of --rounds rounds, the implementations
alternating within each round.

    workloads: 10^5 documents of 180 tokens (13.8 GB of rows) and 10^6 documents of 25 tokens (19.2 GB), generated on the device

    plain       bert_hip_token_index_search_device on an index without removals: token_index_scan_kernel<F16Form, false, false>
    parent      the same call through ANOTHER build of the library (--parent-lib PATH: the commit before the life cycle), its own context
                and its own copy of the same rows: the check that the plain path did not change, against the spread the run shows
    masked all  bert_hip_late_index_search_filtered_device with every document allowed: the mask's cost
    allow ...   a random 10 %, a random 1 % and a contiguous 1 % of the documents allowed: time against the share of allowed tokens
    compact     bert_hip_late_index_compact after a random 10 % of the documents were removed: wall time of the blocking call, the
                gather kernel's own time from the engine's profile, GB/s of live bytes read + written
    save, load  at --file-scale of the workloads (default 0.25: 3.5 and 4.8 GB), into --tmp: wall time and GB/s of the file's bytes

    python tools/late_index_rate.py [--parent-lib PATH] [--scale 1.0] [--file-scale 0.25] [--rounds 3] [--budget-ms 400] [--nq 1,8,64]
                                    [--tmp DIR] [--out profiles/late_index_rate.txt]

The results of every filtered search are checked: masked all == plain == parent in bits; an allow-list's ids are all allowed."""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--file-scale", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget-ms", type=float, default=400.0)
    ap.add_argument("--nq", default="1,8,64")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("late_index_rate.py needs a GPU")
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

    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        path = os.path.join(tmp, "tiny.bin")
        gf.make_synthetic_model(path, "tiny", "f16", seed=0)        # (a context to launch from: the kernels do not read the model)
        m = pybert.BertModel(path)
        P = pctx = None
        if a.parent_lib:
            P = C.CDLL(a.parent_lib)
            # (only what is called here: an older build does not export everything the binding declares)
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            P.bert_load_from_file.restype = vp; P.bert_load_from_file.argtypes = [C.c_char_p]
            P.bert_free.restype = None; P.bert_free.argtypes = [vp]
            P.bert_hip_token_index_create.restype = vp; P.bert_hip_token_index_create.argtypes = [vp, i32]
            P.bert_hip_token_index_free.restype = None; P.bert_hip_token_index_free.argtypes = [vp]
            P.bert_hip_token_index_reserve.restype = i32; P.bert_hip_token_index_reserve.argtypes = [vp, i32, i64, i32, i32, i32]
            P.bert_hip_token_index_add_device.restype = i32; P.bert_hip_token_index_add_device.argtypes = [vp, i32, vp, vp, vp]
            P.bert_hip_token_index_search_device.restype = i32
            P.bert_hip_token_index_search_device.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp]
            pctx = P.bert_load_from_file(path.encode())
            assert pctx, "the parent library could not load the model"
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(1)
        H, lq, k = 384, 32, 10
        unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
        out(f"# token index life cycle, f16 rows, dim {H}, queries of {lq} tokens, k = {k}; {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
            f"us per call = median (min .. max) of {a.rounds} rounds between device events, implementations alternating; scale {a.scale}; "
            f"parent library: {'yes' if P else 'not given'}")
        stream = torch.cuda.current_stream().cuda_stream
        nqs = [int(x) for x in a.nq.split(",")]
        for n_docs, ld in ((int(100000 * a.scale), 180), (int(1000000 * a.scale), 25)):
            n_tok = n_docs * ld
            d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
            for t0 in range(0, n_tok, 1 << 20):
                d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
            dcu_h = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
            ix = m.token_index(H)
            ix.reserve(n_docs, n_tok, max(nqs), lq, k)
            assert ix.add_device(dcu_h, d.data_ptr(), stream) == 0
            pix = None
            if P:
                pix = P.bert_hip_token_index_create(pctx, H)
                assert pix and P.bert_hip_token_index_reserve(pix, n_docs, n_tok, max(nqs), lq, k) == 0
                assert P.bert_hip_token_index_add_device(pix, n_docs, dcu_h.ctypes.data, d.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            n_words = (n_docs + 31) // 32
            rng = np.random.default_rng(2)
            c0 = n_docs // 3
            masks = {"masked all": np.ones(n_docs, bool), "allow random 10 %": rng.random(n_docs) < 0.10, "allow random 1 %": rng.random(n_docs) < 0.01,
                     "allow contiguous 1 %": (np.arange(n_docs) >= c0) & (np.arange(n_docs) < c0 + n_docs // 100)}
            words = {name: torch.from_numpy(pybert.allow_words(mk, n_docs).view(np.int32)).to(dev) for name, mk in masks.items()}
            out(f"# {n_docs} documents of {ld} tokens, {n_tok * H * 2 / 1e9:.1f} GB of rows")
            out("#   case                     nq | allowed share |      us (min .. max)      | / plain | GB/s of allowed rows x nq")
            for nq in nqs:
                q = unit(nq * lq)
                qcu = torch.arange(0, nq + 1, dtype=torch.int32, device=dev) * lq
                res = {name: (torch.empty(nq, k, dtype=torch.int32, device=dev), torch.empty(nq, k, dtype=torch.float32, device=dev))
                       for name in ["plain", "parent"] + list(masks)}

                def plain():
                    ix.search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, res["plain"][0].data_ptr(), res["plain"][1].data_ptr(), stream)

                def parent():
                    r = P.bert_hip_token_index_search_device(pix, nq, qcu.data_ptr(), q.data_ptr(), lq, k, res["parent"][0].data_ptr(),
                                                             res["parent"][1].data_ptr(), stream)
                    assert r == 0

                def filtered(name):
                    def f():
                        ix.search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, res[name][0].data_ptr(), res[name][1].data_ptr(), stream,
                                         words[name].data_ptr(), n_words)
                    return f

                impls = {"plain": plain}
                if P:
                    impls["parent"] = parent
                for name in masks:
                    impls[name] = filtered(name)
                t = measure(impls)
                torch.cuda.synchronize()
                same = lambda x, y: torch.equal(res[x][0], res[y][0]) and torch.equal(res[x][1], res[y][1])
                assert same("masked all", "plain"), "the masked scan with every document allowed is not the plain search"
                assert not P or same("parent", "plain"), "the plain search is not the parent's"
                for name, mk in masks.items():
                    got = res[name][0].cpu().numpy()
                    assert (got >= 0).all() and mk[got].all(), name
                base = t["plain"][0]
                for name in impls:
                    share = 1.0 if name in ("plain", "parent") else float(masks[name].mean())
                    us, lo, hi = t[name]
                    out(f"    {name:24s} {nq:4d} | {share:13.4f} | {us:10.1f} ({lo:.1f} .. {hi:.1f}) | {us / base:7.3f} | {nq * share * n_tok * H * 2 / (us * 1e-6) / 1e9:10.1f}")
            if pix:
                P.bert_hip_token_index_free(pix)
            # compact after removing a random 10 %
            gone = np.flatnonzero(rng.random(n_docs) < 0.10).astype(np.int32)
            t0 = time.perf_counter()
            assert ix.remove(gone) == len(gone)
            t_remove = time.perf_counter() - t0
            live_bytes = ix.n_live_tokens() * H * 2
            m.profile_report()
            m.profile(True)
            t0 = time.perf_counter()
            old = ix.compact()
            t_compact = time.perf_counter() - t0
            m.profile(False)
            gather_ms = m.profile_report().get("token_index_gather", {}).get("total_ms", float("nan"))
            assert len(old) == n_docs - len(gone) == len(ix) and ix.n_tokens() * H * 2 == live_bytes
            out(f"    remove {len(gone)} documents: {t_remove * 1e3:.1f} ms (blocking, the first remove: the bitmap is made)")
            out(f"    compact to {len(ix)} documents, {live_bytes / 1e9:.2f} GB live: {t_compact * 1e3:.1f} ms wall (allocation, gather, release), "
                f"{2 * live_bytes / t_compact / 1e9:.0f} GB/s read + written; token_index_gather_kernel alone {gather_ms:.2f} ms, "
                f"{2 * live_bytes / (gather_ms * 1e-3) / 1e9:.0f} GB/s read + written")
            ix.close()
            # save and load at the file scale
            nf = max(1, int(n_docs * a.file_scale))
            fx = m.token_index(H)
            assert fx.add_device(dcu_h[:nf + 1], d.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            fx.remove(np.flatnonzero(rng.random(nf) < 0.10).astype(np.int32))
            fpath = os.path.join(tmp, "index.tok")
            try:
                t0 = time.perf_counter()
                fx.save(fpath)
                t_save = time.perf_counter() - t0
                size = os.path.getsize(fpath)
                t0 = time.perf_counter()
                back = m.load_token_index(fpath)
                t_load = time.perf_counter() - t0
                assert len(back) == nf and back.n_live() == fx.n_live()
                back.close()
                out(f"    save {nf} documents ({size / 1e9:.2f} GB, removals kept): {t_save:.2f} s, {size / t_save / 1e9:.2f} GB/s; "
                    f"load (just written: from the page cache where it fits): {t_load:.2f} s, {size / t_load / 1e9:.2f} GB/s")
            except RuntimeError as e:
                out(f"    save / load of {nf} documents: not measured ({e})")
            if os.path.exists(fpath):
                os.remove(fpath)
            fx.close()
            del d
            torch.cuda.empty_cache()
        if P:
            P.bert_free(pctx)
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
