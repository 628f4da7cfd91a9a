#!/usr/bin/env python3
"""Rate of the int8 token index's MASKED scan, which tools/late_i8_rate.py does not reach: bert_hip_late_index_search_filtered_device with
every document allowed, by late_i8_rate.py's method — dim 384 and 128, its two workloads, 1 / 8 / 64 queries of 32 tokens, k = 10, the
median (min .. max) us per call of 3 rounds between device events.  For comparing two builds of the library (BERT_HIP_LIB) in
alternating processes:

    python tools/late_i8_masked_rate.py"""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
os.environ.setdefault("BERT_HIP_QUIET", "1")
from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert


def timed(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "tiny.bin")
    gf.make_synthetic_model(path, "tiny", "f16", seed=0)
    m = pybert.BertModel(path)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    lq, k = 32, 10
    stream = torch.cuda.current_stream().cuda_stream
    for H in (384, 128):
        unit = lambda n: torch.nn.functional.normalize(torch.randn(n, H, generator=gen, device=dev), dim=1).to(torch.float16)
        for n_docs, ld in ((100000, 180), (1000000, 25)):
            n_tok = n_docs * ld
            d = torch.empty(n_tok, H, dtype=torch.float16, device=dev)
            for t0 in range(0, n_tok, 1 << 20):
                d[t0:t0 + (1 << 20)] = unit(min(1 << 20, n_tok - t0))
            cu = (np.arange(n_docs + 1, dtype=np.int64) * ld).astype(np.int32)
            ix = m.token_index(H, "i8")
            ix.reserve(n_docs, n_tok, 64, lq, k)
            assert ix.add_device(cu, d.data_ptr(), stream) == 0
            nw = (n_docs + 31) // 32
            allow = torch.full((nw,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for nq in (1, 8, 64):
                q = unit(nq * lq)
                qcu = torch.arange(0, nq + 1, dtype=torch.int32, device=dev) * lq
                ids = torch.empty(nq, k, dtype=torch.int32, device=dev); sc = torch.empty(nq, k, dtype=torch.float32, device=dev)
                f = lambda: ix.search_device(nq, qcu.data_ptr(), q.data_ptr(), lq, k, ids.data_ptr(), sc.data_ptr(), stream, allow.data_ptr(), nw)
                f(); torch.cuda.synchronize()
                once = timed(f, 1)
                iters = int(max(2, min(200, 300e3 / max(once, 1.0))))
                t = [timed(f, iters) for _ in range(3)]
                print(f"masked int8 scan {n_docs:8d} x {ld:3d} dim {H:4d} nq {nq:3d} | {np.median(t):10.1f} ({min(t):.1f} .. {max(t):.1f})", flush=True)
            ix.close(); del d; torch.cuda.empty_cache()
    m.close()
