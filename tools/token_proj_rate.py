#!/usr/bin/env python3
"""Rate of the projection head over token rows (csrc/token_proj.hip) on one GPU:

    models     768 -> 128 (bert-base dims, 12 layers) and 384 -> 96 (minilm-l6 dims), synthetic f16 files with a random head
    batches    256 sentences x 128 tokens and 4096 x 25 tokens
    (a) the projection launch ("token_project" of the engine's profile, projected + normalised + f16) against the copy it replaces
        ("token_rows", normalised + f16, of the same call without flag bit 2), against torch matmul + normalize on f16 rows of the
        same shape, and against the bytes it must move, T H 2 read + T P 2 written, at the HBM line (--hbm-tbs, 8 TB/s)
    (b) the whole device call bert_hip_eval_packed_tokens_device with flags 1 | 2 | 4 against flags 1 | 2
    (c) bert_hip_token_index_add_texts into an index at the head's dim against one at n_embd, the same texts

    python tools/token_proj_rate.py [--rounds 5] [--scale 1.0] [--out profiles/token_proj_rate.txt]

One process.  (b) and torch: device events around back-to-back calls; (a): the profile's per-launch events, a run of its own; (c): a
host clock around the blocking call into a fresh index.  The arms are interleaved within each round; a figure is the FASTEST of
--rounds rounds with min .. max beside it.  --scale shrinks the sentence counts (a smoke run)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("token_proj_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def events(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def rounds(arms):
        """arms: name -> callable returning us; (fastest, min, max) per name, interleaved"""
        t = {n: [] for n in arms}
        for n, f in arms.items():
            f()                                               # warm-up of every arm
        for _ in range(a.rounds):
            for n, f in arms.items():
                t[n].append(f())
        return {n: (min(v), min(v), max(v)) for n, v in t.items()}

    cell = lambda v: f"{v[0]:9.1f} ({v[1]:.1f} .. {v[2]:.1f})"
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    out(f"# projection head over token rows; {torch.cuda.get_device_name(0)}, torch {torch.__version__}; us = fastest (min .. max) of {a.rounds} rounds, arms "
        f"interleaved; HBM line {a.hbm_tbs} TB/s; scale {a.scale}")
    with tempfile.TemporaryDirectory() as tmp:
        for dims, P in (("bert-base", 128), ("minilm-l6", 96)):
            hp = gf.MODEL_DIMS[dims]
            H = hp.n_embd
            w = gf.synthetic_weights(hp, seed=1)
            w[gf.TOKEN_PROJ_NAME] = np.random.default_rng(2).normal(0, 1 / np.sqrt(H), (P, H)).astype(np.float32)
            path = os.path.join(tmp, f"{dims}.bin")
            vocab = [f"w{i}".encode() for i in range(hp.n_vocab)]
            vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]", b"[MASK]"
            gf.write_model(path, hp, w, gf.FTYPE_F16, vocab=vocab)
            del w
            m = pybert.BertModel(path)
            for B, L in ((max(1, int(256 * a.scale)), 128), (max(1, int(4096 * a.scale)), 25)):
                T = B * L
                toks = torch.from_numpy(gf.synthetic_token_ids(B, L, hp.n_vocab, seed=3).reshape(-1).astype(np.int32)).to(dev)
                cu = (torch.arange(B + 1, dtype=torch.int32) * L).to(dev)
                rows = torch.empty(T, H, dtype=torch.float16, device=dev)
                m.reserve(T, B)
                call = lambda project: m.eval_packed_tokens_device(toks.data_ptr(), cu.data_ptr(), B, T, L, rows.data_ptr(), None, True, True, stream, project)

                def launch_us(project, name):
                    m.profile(True)
                    before = m.profile_report().get(name, {"launches": 0, "total_ms": 0.0})
                    for _ in range(10):
                        call(project)
                    torch.cuda.synchronize()
                    after = m.profile_report()[name]
                    m.profile(False)
                    n = after["launches"] - before["launches"]
                    return (after["total_ms"] - before["total_ms"]) * 1e3 / n if n > 0 else after["total_ms"] * 1e3 / after["launches"]

                x = torch.randn(T, H, device=dev).to(torch.float16)
                wp = torch.randn(P, H, device=dev).to(torch.float16) / H ** 0.5
                torch_arm = lambda: events(lambda: torch.nn.functional.normalize(x @ wp.T, dim=1), 20)
                t = rounds({"project": lambda: launch_us(True, "token_project"), "rows": lambda: launch_us(False, "token_rows"), "torch": torch_arm,
                            "call4": lambda: events(lambda: call(True), 5), "call": lambda: events(lambda: call(False), 5)})
                floor = (T * H * 2 + T * P * 2) / (a.hbm_tbs * 1e12) * 1e6
                out(f"{H} -> {P}, {B} x {L} tokens (T = {T}):")
                out(f"  (a) token_project {cell(t['project'])} us | token_rows (no head) {cell(t['rows'])} us | torch matmul + normalize {cell(t['torch'])} us | "
                    f"torch / token_project {t['torch'][0] / t['project'][0]:.2f} | bytes at the HBM line {floor:.1f} us = {100 * floor / t['project'][0]:.0f} % of the launch")
                out(f"  (b) call with flag 4 {cell(t['call4'])} us | call without {cell(t['call'])} us | with / without {t['call4'][0] / t['call'][0]:.3f}")
                del x, rows
            # (c) texts of 23 words (25 tokens): into an index at P against one at H
            n_txt = max(1, int(4096 * a.scale))
            rng = np.random.default_rng(4)
            texts = [" ".join(f"w{i}" for i in rng.integers(1000, hp.n_vocab, 23)) for _ in range(n_txt)]

            def add_us(dim):
                ix = m.token_index(dim)
                ix.reserve(n_txt, n_txt * 25)
                t0 = time.perf_counter()
                ix.add_texts(texts)
                dt = (time.perf_counter() - t0) * 1e6
                ix.close()
                return dt

            t = rounds({"P": lambda: add_us(P), "H": lambda: add_us(H)})
            out(f"{H} -> {P}, add_texts of {n_txt} texts x 25 tokens:")
            out(f"  (c) index at dim {P} {cell(t['P'])} us | index at dim {H} {cell(t['H'])} us | P / H {t['P'][0] / t['H'][0]:.3f}")
            m.close()
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
