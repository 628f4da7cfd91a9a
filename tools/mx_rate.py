#!/usr/bin/env python3
"""Rate of the MXFP8 forward route ("mx" = 1: gemm_mx.hip) beside the f16 route ("mx" = 0) of the SAME context, loaded with
BERT_HIP_MX=fp8 — one process, one GPU, a synthetic model of bert-base's dimensions (BASELINE configs[3]):

    python tools/mx_rate.py [--sentences 512] [--len 512] [--rounds 5] [--out profiles/mx_rate.txt]

The whole pass: device events around one bert_hip_eval_packed_device call per setting, the two settings alternating within a round,
the FASTEST of --rounds rounds with (min .. max).  The four weight mat-muls, the quantise launches and the rest: the engine's own
per-launch times (bert_hip_profile_report) of one profiled pass per setting, as milliseconds per layer.  No threshold: what comes out."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMS = ("gemm_qkv", "gemm_attn_out", "gemm_ffn_up", "gemm_ffn_down")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=512)
    ap.add_argument("--len", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dims", default="bert-base")
    ap.add_argument("--model-dir", default="/tmp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mx_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    os.environ["BERT_HIP_MX"] = "fp8"
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    path = os.path.join(a.model_dir, f"mx_rate_{a.dims}_f16.bin")
    hp = gf.make_synthetic_model(path, a.dims, "f16", seed=1)
    m = pybert.BertModel(path)
    B, n, T, H = a.sentences, a.len, a.sentences * a.len, hp.n_embd
    rng = np.random.default_rng(0)
    toks = torch.from_numpy(rng.integers(0, hp.n_vocab, size=T).astype(np.int32)).cuda()
    cu = torch.from_numpy((np.arange(B + 1) * n).astype(np.int32)).cuda()
    res = torch.empty((B, H), dtype=torch.float32, device="cuda")
    m.reserve(T, B)

    def run():
        m.eval_packed_device(toks.data_ptr(), cu.data_ptr(), B, T, n, res.data_ptr(), 0)

    def timed_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    emb, t, prof = {}, {"0": [], "1": []}, {}
    for mx in ("0", "1"):                                     # warm-up, the embeddings, one profiled pass
        m.set_option("mx", mx)
        run(); torch.cuda.synchronize()
        emb[mx] = res.cpu().numpy().astype(np.float64)
        m.profile(True); run(); prof[mx] = m.profile_report(families=True); m.profile(False)
    for _ in range(a.rounds):
        for mx in ("0", "1"):
            m.set_option("mx", mx)
            t[mx].append(timed_ms())
    out(f"mx_rate: {a.dims} dims, {B} sentences x {n} tokens = {T} tokens, {hp.n_layer} layers, {torch.cuda.get_device_name(0)}")
    for mx in ("0", "1"):
        fam = sorted(k for k in prof[mx] if k.startswith("family:"))
        out(f"pass mx = {mx}: {min(t[mx]):9.3f} ms ({min(t[mx]):.3f} .. {max(t[mx]):.3f}) = {B / min(t[mx]) * 1e3:9.1f} sentences/s   {' '.join(fam)}")
    out(f"pass: mx = 1 takes {min(t['1']) / min(t['0']):.3f} of mx = 0's time")
    per_layer = lambda rep, k: rep[k]["total_ms"] / hp.n_layer if k in rep else 0.0
    for k in GEMMS:
        t0, t1 = per_layer(prof["0"], k), per_layer(prof["1"], k)
        fl = prof["1"][k]["flops_per_launch"]
        out(f"{k:14s} per layer: mx = 0 {t0:8.3f} ms ({fl / t0 / 1e9 if t0 else 0:7.1f} TFLOP/s)   mx = 1 {t1:8.3f} ms ({fl / t1 / 1e9:7.1f} TFLOP/s)   ratio {t1 / t0 if t0 else float('nan'):.3f}")
    total1 = sum(v["total_ms"] for k, v in prof["1"].items() if not k.startswith("family:"))
    q = prof["1"]["mx_quantize"]
    out(f"mx_quantize: {q['launches']} launches, {q['total_ms']:.3f} ms = {q['total_ms'] / total1:.3f} of the launches' {total1:.3f} ms (mx = 1)")
    for mx in ("0", "1"):
        rest = {k: v["total_ms"] for k, v in prof[mx].items() if not k.startswith("family:") and k not in GEMMS and k != "mx_quantize"}
        out(f"others mx = {mx}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in sorted(rest.items())))
    cos = (emb["0"] * emb["1"]).sum(1) / np.linalg.norm(emb["0"], axis=1) / np.linalg.norm(emb["1"], axis=1)
    out(f"cosine mx = 1 against mx = 0 per sentence (synthetic weights): worst {cos.min():.6f} mean {cos.mean():.6f}")
    m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
