"""Rate of the embedding index's search (bert_hip_index_search_device) on one GPU, with torch's matmul + topk on the same
device and data beside every line as the yardstick, and the rate of bert_hip_index_add_texts against bert_encode_batch +
bert_hip_index_add.  GPU only: there is no CPU fallback.

    python tools/search_rate.py [--rows 1000000] [--iters 10] [--out profiles/search_rate.txt]
                                [--sections search,filter,texts] [--dims 384,768] [--dtypes f16,f32,i8] [--no-yardstick]
    python tools/search_rate.py --sections rescore --out profiles/search_b1_rate.txt

Per line: ms per call (device events, after warm-up), queries/s, the algorithmic bytes (the rows once, the queries, the
results) and FLOPs (2 Q N dim), the share of the binding roofline (HBM 6.3 TB/s achievable; matrix cores 2.5 PF/s f16,
155 TF/s f32, 5 PF/s i8) and its name, torch's ms, and whether the two agree (per query: the same ids up to ties within
tolerance).  i8 rows count dpad + 4 bytes (codes and scale); torch's yardstick for them is the same quantization and score
restated in torch (f32 mat-mul of the codes, exact at these dims: every partial sum is an integer below 2^24).  b1 rows
(--dtypes ...,b1) count dpad / 8 bytes with dpad = dim rounded up to 128; their yardstick is the int8 query codes against a
+-1 matrix of the rows' sign bits, times the query scale; their matrix-core line is the i8 one.

Section "filter" (bert_hip_index_search_filtered_device; f16 and i8 rows, dim 384, k = 10, Q = 1 and 4096): the unfiltered
call, then allow-lists of density 1.0, 0.1 and 0.01, with the allowed rows drawn at random or in contiguous runs of 4096 rows
spread evenly over the index.  Per line: ms per call (median, and the smallest and largest of the iterations: the run-to-run
spread), the ratio to the unfiltered line, and the rows that qualify.  --no-yardstick leaves torch's column out (for a quick
comparison of two builds).

Section "rescore" (not part of the default; 10^6 rows, dims 384 and 768, Q = 1 and 4096, k = 10): the b1 search, the two-stage
search b1(100) -> i8 (bert_hip_index_search_rescored_device) and the plain i8 search, from the same run on the same box, each as
median (min .. max), and the share of the two-stage answers' ids that the plain i8 search also returns.

Section "probe" (not part of the default; a clustered corpus of 10^6 rows — 4096 random centres, unit rows of centre + noise —,
dim 384, f16 and i8 rows, n_lists = 1024, Q = 1 and 4096, k = 10): the time of BertIndex.train_partition, then the plain search
and the probed search (bert_hip_index_search_probed_device) with nprobe = 1, 8, 32, 128 from the same run, each as median
(min .. max) and as a ratio to the plain line, with recall@10 against the plain search's ids beside it.
    python tools/search_rate.py --sections probe --out profiles/search_probe_rate.txt

Section "probe_filter" (not part of the default; the corpus and the partition of "probe", f16 and i8 rows, nprobe = 8, Q = 1 and
4096, k = 10): the probed search without a list (bert_hip_index_search_probed_device), then
bert_hip_index_search_probed_filtered_device with allow-lists of density 1.0, 0.1 and 0.01 (rows allowed at random), each as
median (min .. max) and as a ratio to the unfiltered probed line of the same run.
    python tools/search_rate.py --sections probe_filter --out profiles/search_probe_filter_rate.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
PEAK = {"f16": 2.5e15, "f32": 155e12, "i8": 5.0e15, "b1": 5.0e15}


def agree(ids, scores, t_ids, t_vals, k, tol):
    """set equality up to ties: every id that only one side returned scores within tol of that side's k-th score"""
    for q in range(ids.shape[0]):
        a, b = set(ids[q].tolist()), set(t_ids[q].tolist())
        if a == b:
            continue
        if not (abs(float(scores[q, k - 1]) - float(t_vals[q, k - 1])) <= tol and
                all(float(scores[q, list(ids[q]).index(i)]) <= float(scores[q, k - 1]) + tol for i in a - b) and
                all(float(t_vals[q, list(t_ids[q]).index(i)]) <= float(t_vals[q, k - 1]) + tol for i in b - a)):
            return False
    return True


def quantize(x):
    """the i8 index's quantizer (include/bert_hip.h), restated in torch: codes as f32 and one scale per row"""
    import torch
    scale = x.abs().amax(dim=1) / 127
    codes = torch.clamp(torch.round(x / scale[:, None]), -127, 127)
    return torch.where(scale[:, None] == 0, torch.zeros_like(codes), codes), scale


def filter_section(a, m, N, out, timed, torch, dev, sp):
    """search_filtered_device against search_device on the same index: what an allow-list costs or saves"""
    from bert_cpp_amd import pybert
    dim, k, run = 384, 10, 4096
    out(f"# search_filtered_device, N = {N} rows, dim {dim}, k = {k}; allow-list of the given density, rows allowed at random or in "
        f"contiguous runs of {run} rows; ms = median (min .. max) of {a.iters}")
    out("# dtype     Q  allow-list          qualifying |      ms (min .. max)        x unfiltered")
    g = torch.Generator(device=dev).manual_seed(dim)
    C = torch.randn(N, dim, device=dev, generator=g)
    C /= C.norm(dim=1, keepdim=True)
    Qall = torch.randn(4096, dim, device=dev, generator=g)
    Qall /= Qall.norm(dim=1, keepdim=True)
    rng = np.random.default_rng(1)
    lists = [("none (search_device)", None)]
    for density in (1.0, 0.1, 0.01):
        if density == 1.0:
            lists.append(("1.0", np.ones(N, bool)))
            continue
        lists.append((f"{density} random", rng.random(N) < density))
        blocks = np.zeros(N, bool)
        n_runs = max(1, int(round(density * N / run)))
        for start in np.linspace(0, N - run, n_runs).astype(np.int64) // 128 * 128:
            blocks[start:start + run] = True
        lists.append((f"{density} contiguous", blocks))
    for dtype in ("f16", "i8"):
        ix = m.index(dim=dim, dtype=dtype)
        ix.reserve(N, 4096, k)
        ix.add_device(N, C.data_ptr(), sp)
        for Q in (1, 4096):
            q = Qall[:Q].contiguous()
            ids = torch.empty(Q, k, dtype=torch.int32, device=dev)
            sc = torch.empty(Q, k, dtype=torch.float32, device=dev)
            base = None
            for name, keep in lists:
                if keep is None:
                    t, lo, hi = timed(lambda: ix.search_device(Q, q.data_ptr(), k, ids.data_ptr(), sc.data_ptr(), sp))
                    base, n_q = t, N
                else:
                    words = torch.from_numpy(pybert.allow_words(keep, N).view(np.int32)).to(dev)
                    t, lo, hi = timed(lambda: ix.search_device(Q, q.data_ptr(), k, ids.data_ptr(), sc.data_ptr(), sp,
                                                               d_allow_ptr=words.data_ptr(), n_words=words.numel()))
                    n_q = int(keep.sum())
                    # (every returned row is an allowed one)
                    got = ids.cpu().numpy()
                    assert keep[got[got >= 0]].all(), name
                out(f"{dtype:7s} {Q:5d}  {name:20s} {n_q:9d} | {t:8.3f} ({lo:7.3f} .. {hi:7.3f})  {t / base:6.2f}")
        ix.close()


def rescore_section(a, m, N, out, timed, torch, dev, sp):
    """the b1 search, b1(100) -> i8 two-stage and the plain i8 search side by side"""
    k, n_cand = 10, 100
    out(f"# b1 search, b1({n_cand}) -> i8 two-stage search and i8 search, N = {N} rows, k = {k}; ms = median (min .. max) of {a.iters}")
    out("#  dim     Q  call                    |      ms (min .. max)        queries/s   ids shared with i8")
    for dim in (384, 768):
        g = torch.Generator(device=dev).manual_seed(dim)
        C = torch.randn(N, dim, device=dev, generator=g)
        C /= C.norm(dim=1, keepdim=True)
        Qall = torch.randn(4096, dim, device=dev, generator=g)
        Qall /= Qall.norm(dim=1, keepdim=True)
        b1, i8 = m.index(dim=dim, dtype="b1"), m.index(dim=dim, dtype="i8")
        for ix, kk in ((b1, n_cand), (i8, k)):
            ix.reserve(N, 4096, kk)
            ix.add_device(N, C.data_ptr(), sp)
        for Q in (1, 4096):
            q = Qall[:Q].contiguous()
            ids = {name: torch.empty(Q, k, dtype=torch.int32, device=dev) for name in ("b1", "two-stage", "i8")}
            sc = torch.empty(Q, k, dtype=torch.float32, device=dev)
            calls = {"b1": lambda: b1.search_device(Q, q.data_ptr(), k, ids["b1"].data_ptr(), sc.data_ptr(), sp),
                     "two-stage": lambda: b1.search_rescored_device(i8, Q, q.data_ptr(), n_cand, k, ids["two-stage"].data_ptr(), sc.data_ptr(), sp),
                     "i8": lambda: i8.search_device(Q, q.data_ptr(), k, ids["i8"].data_ptr(), sc.data_ptr(), sp)}
            times = {name: timed(f) for name, f in calls.items()}
            want = ids["i8"].cpu().numpy()
            for name, label in (("b1", "b1 search"), ("two-stage", f"b1({n_cand}) -> i8"), ("i8", "i8 search")):
                t, lo, hi = times[name]
                got = ids[name].cpu().numpy()
                shared = np.mean([len(set(x.tolist()) & set(y.tolist())) / k for x, y in zip(got, want)])
                out(f"{dim:6d} {Q:5d}  {label:22s} | {t:8.3f} ({lo:7.3f} .. {hi:7.3f}) {Q / (t * 1e-3):11.0f}   {shared:.3f}")
        b1.close()
        i8.close()
        del C, Qall
        torch.cuda.empty_cache()


def probe_section(a, m, N, out, timed, torch, dev, sp):
    """the plain search and the probed search of a partitioned index side by side, with the recall of the probed one"""
    dim, k, n_lists, n_centres, sigma = 384, 10, 1024, 4096, 0.04
    out(f"# search_probed_device against search_device, N = {N} rows in {n_centres} clusters (unit rows of centre + {sigma} * noise), dim {dim}, "
        f"n_lists = {n_lists}, k = {k}; ms = median (min .. max) of {a.iters}; recall@{k} against the plain search's ids")
    out("# dtype     Q  call            |      ms (min .. max)        x plain   queries/s   recall")
    g = torch.Generator(device=dev).manual_seed(dim)
    centres = torch.randn(n_centres, dim, device=dev, generator=g)
    centres /= centres.norm(dim=1, keepdim=True)

    def draw(n):
        x = centres[torch.randint(0, n_centres, (n,), device=dev, generator=g)] + sigma * torch.randn(n, dim, device=dev, generator=g)
        return x / x.norm(dim=1, keepdim=True)

    C, Qall = draw(N), draw(4096)
    for dtype in ("f16", "i8"):
        ix = m.index(dim=dim, dtype=dtype)
        ix.reserve(N, 4096, k)
        ix.add_device(N, C.data_ptr(), sp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ix.train_partition(n_lists, n_iter=10, seed=0)
        lens = np.bincount(ix.partition_lists(), minlength=n_lists)
        out(f"# {dtype}: train_partition({n_lists}, n_iter=10) {time.perf_counter() - t0:.2f} s; list lengths min {lens.min()}, "
            f"median {int(np.median(lens))}, max {lens.max()}")
        for Q in (1, 4096):
            q = Qall[:Q].contiguous()
            ids = torch.empty(Q, k, dtype=torch.int32, device=dev)
            pid = torch.empty(Q, k, dtype=torch.int32, device=dev)
            sc = torch.empty(Q, k, dtype=torch.float32, device=dev)
            base, lo, hi = timed(lambda: ix.search_device(Q, q.data_ptr(), k, ids.data_ptr(), sc.data_ptr(), sp))
            want = ids.cpu().numpy()
            out(f"{dtype:7s} {Q:5d}  {'search':15s} | {base:8.3f} ({lo:7.3f} .. {hi:7.3f})  {1.0:6.2f} {Q / (base * 1e-3):11.0f}   1.000")
            for nprobe in (1, 8, 32, 128):
                t, lo, hi = timed(lambda: ix.search_probed_device(Q, q.data_ptr(), nprobe, k, pid.data_ptr(), sc.data_ptr(), sp))
                got = pid.cpu().numpy()
                recall = np.mean([len(set(x.tolist()) & set(y.tolist())) / k for x, y in zip(got, want)])
                out(f"{dtype:7s} {Q:5d}  {'nprobe = %d' % nprobe:15s} | {t:8.3f} ({lo:7.3f} .. {hi:7.3f})  {t / base:6.2f} {Q / (t * 1e-3):11.0f}   {recall:.3f}")
        ix.close()


def probe_filter_section(a, m, N, out, timed, torch, dev, sp):
    """search_probed_filtered_device against search_probed_device on the same partitioned index: what an allow-list costs or saves"""
    from bert_cpp_amd import pybert
    dim, k, n_lists, n_centres, sigma, nprobe = 384, 10, 1024, 4096, 0.04, 8
    out(f"# search_probed_filtered_device against search_probed_device, N = {N} rows in {n_centres} clusters (unit rows of centre + {sigma} * noise), "
        f"dim {dim}, n_lists = {n_lists}, nprobe = {nprobe}, k = {k}; allow-list of the given density, rows allowed at random; "
        f"ms = median (min .. max) of {a.iters}")
    out("# dtype     Q  allow-list                    qualifying |      ms (min .. max)        x unfiltered probed")
    g = torch.Generator(device=dev).manual_seed(dim)
    centres = torch.randn(n_centres, dim, device=dev, generator=g)
    centres /= centres.norm(dim=1, keepdim=True)

    def draw(n):
        x = centres[torch.randint(0, n_centres, (n,), device=dev, generator=g)] + sigma * torch.randn(n, dim, device=dev, generator=g)
        return x / x.norm(dim=1, keepdim=True)

    C, Qall = draw(N), draw(4096)
    rng = np.random.default_rng(1)
    lists = [("none (search_probed_device)", None)] + [(f"{d}" + ("" if d == 1.0 else " random"), np.ones(N, bool) if d == 1.0 else rng.random(N) < d)
                                                       for d in (1.0, 0.1, 0.01)]
    cents = None
    for dtype in ("f16", "i8"):
        ix = m.index(dim=dim, dtype=dtype)
        ix.reserve(N, 4096, k)
        ix.add_device(N, C.data_ptr(), sp)
        torch.cuda.synchronize()
        # (the centroids are trained once, on the f16 rows, and installed into both indexes)
        if cents is None:
            cents = ix.train_partition(n_lists, n_iter=10, seed=0)
        else:
            ix.partition(cents)
        for Q in (1, 4096):
            q = Qall[:Q].contiguous()
            ids = torch.empty(Q, k, dtype=torch.int32, device=dev)
            sc = torch.empty(Q, k, dtype=torch.float32, device=dev)
            base = None
            for name, keep in lists:
                if keep is None:
                    t, lo, hi = timed(lambda: ix.search_probed_device(Q, q.data_ptr(), nprobe, k, ids.data_ptr(), sc.data_ptr(), sp))
                    base, n_q = t, N
                else:
                    words = torch.from_numpy(pybert.allow_words(keep, N).view(np.int32)).to(dev)
                    t, lo, hi = timed(lambda: ix.search_probed_device(Q, q.data_ptr(), nprobe, k, ids.data_ptr(), sc.data_ptr(), sp,
                                                                      d_allow_ptr=words.data_ptr(), n_words=words.numel()))
                    n_q = int(keep.sum())
                    # (every returned row is an allowed one)
                    got = ids.cpu().numpy()
                    assert keep[got[got >= 0]].all(), name
                out(f"{dtype:7s} {Q:5d}  {name:29s} {n_q:9d} | {t:8.3f} ({lo:7.3f} .. {hi:7.3f})  {t / base:6.2f}")
        ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="search,filter,texts")
    ap.add_argument("--dims", default="384,768")
    ap.add_argument("--dtypes", default="f16,f32,i8")
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    import torch
    torch.backends.cuda.matmul.allow_tf32 = False
    if not torch.cuda.is_available():
        sys.exit("search_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "minilm.bin")
    gf.make_synthetic_model(path, "minilm-l6", "f16", seed=1)
    m = pybert.BertModel(path)
    st = torch.cuda.current_stream()
    sp = st.cuda_stream
    N = a.rows
    sections = a.sections.split(",")
    dims = [int(d) for d in a.dims.split(",")] if "search" in sections else []
    dtypes = a.dtypes.split(",")

    def timed(f):
        """ms per call: (median, smallest, largest) of a.iters calls after 3 warm-up calls"""
        for _ in range(3):
            f()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            f()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    out(f"# search_device, N = {N} rows, {torch.cuda.get_device_name(0)}; ms per call = median of {a.iters} after 3 warm-up calls")
    out("# dim dtype     Q    k |      ms (min .. max)       queries/s  bytes      FLOPs   | bound  share | torch ms  agree")
    for dim in dims:
        g = torch.Generator(device=dev).manual_seed(dim)
        C = torch.randn(N, dim, device=dev, generator=g)
        C /= C.norm(dim=1, keepdim=True)
        Qall = torch.randn(4096, dim, device=dev, generator=g)
        Qall /= Qall.norm(dim=1, keepdim=True)
        for dtype in dtypes:
            ix = m.index(dim=dim, dtype=dtype)
            ix.reserve(N, 4096, 100)
            ix.add_device(N, C.data_ptr(), sp)
            Ct = C.half() if dtype == "f16" else C
            if dtype == "i8":
                Ct, Cs = quantize(C)
            if dtype == "b1":
                Ct = torch.where(C > 0, 1.0, -1.0)
            for Q in (1, 16, 256, 4096):
                q = Qall[:Q].contiguous()
                for k in (10, 100):
                    ids = torch.empty(Q, k, dtype=torch.int32, device=dev)
                    sc = torch.empty(Q, k, dtype=torch.float32, device=dev)

                    def call():
                        ix.search_device(Q, q.data_ptr(), k, ids.data_ptr(), sc.data_ptr(), sp)

                    def yard():
                        qt = q.half() if dtype == "f16" else q
                        if dtype in ("i8", "b1"):
                            qt, qs = quantize(q)
                        res = []
                        for c0 in range(0, Q, 256):          # (a [256, N] f32 score block at a time: 1 GB)
                            s = (qt[c0:c0 + 256] @ Ct.T).float()
                            if dtype == "i8":
                                s = (s * qs[c0:c0 + 256, None]) * Cs[None, :]
                            if dtype == "b1":
                                s = s * qs[c0:c0 + 256, None]
                            res.append(torch.topk(s, k, dim=1))
                        return torch.cat([r.values for r in res]), torch.cat([r.indices for r in res])

                    t, t_lo, t_hi = timed(call)
                    ty, ok = float("nan"), None
                    if not a.no_yardstick:
                        ty = timed(yard)[0]
                        tv, ti = yard()
                        torch.cuda.synchronize()
                        nq = min(Q, 64)
                        ok = agree(ids[:nq].cpu().numpy(), sc[:nq].cpu().numpy(), ti[:nq].cpu().numpy(), tv[:nq].cpu().numpy(), k, 1e-3)
                    es = {"f16": 2, "f32": 4, "i8": 1, "b1": 0.125}[dtype]
                    step = {"f16": 16, "f32": 8, "i8": 32, "b1": 128}[dtype]
                    dpad = (dim + step - 1) // step * step
                    nbytes = N * (int(dpad * es) + (4 if dtype == "i8" else 0)) + Q * dim * 4 + Q * k * 8
                    flops = 2.0 * Q * N * dim
                    tb, tf = nbytes / HBM, flops / PEAK[dtype]
                    bound, share = ("HBM", tb / (t * 1e-3)) if tb >= tf else ("MFMA", tf / (t * 1e-3))
                    out(f"{dim:5d} {dtype:5s} {Q:5d} {k:4d} | {t:8.3f} ({t_lo:7.3f} .. {t_hi:7.3f}) {Q / (t * 1e-3):11.0f}  {nbytes:.2e} {flops:.2e} | "
                        f"{bound:5s} {share:6.3f} | {ty:8.3f}  {'-' if ok is None else 'yes' if ok else 'NO'}")
            ix.close()
            del Ct
        del C, Qall
        torch.cuda.empty_cache()

    if "filter" in sections:
        filter_section(a, m, N, out, timed, torch, dev, sp)

    if "rescore" in sections:
        rescore_section(a, m, N, out, timed, torch, dev, sp)

    if "probe" in sections:
        probe_section(a, m, N, out, timed, torch, dev, sp)

    if "probe_filter" in sections:
        probe_filter_section(a, m, N, out, timed, torch, dev, sp)

    # strings in, index rows out: add_texts against encode_batch + add
    if "texts" in sections:
        base = [l.rstrip("\n") for l in open(os.path.join(ROOT, "tests", "golden", "sample_client_texts_600.txt"), encoding="utf-8")]
        texts = [f"{base[i % len(base)]} {i}" for i in range(32768)]
        rates = {}
        for name in ("add_texts", "encode_batch+add"):
            best = 1e9
            for _ in range(3):
                ix = m.index(dtype="f16")
                t0 = time.perf_counter()
                if name == "add_texts":
                    ix.add_texts(texts, n_threads=16)
                else:
                    ix.add(m.encode_batch(texts, n_threads=16))
                best = min(best, time.perf_counter() - t0)
                ix.close()
            rates[name] = len(texts) / best
        out(f"# texts into the index (minilm-l6 synthetic f16, 32768 texts, best of 3): add_texts {rates['add_texts']:.0f} texts/s, "
            f"encode_batch + add {rates['encode_batch+add']:.0f} texts/s")
    m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
