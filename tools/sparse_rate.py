#!/usr/bin/env python3
"""Rate of the learned sparse embeddings (bert_hip_sparse_packed_device) on one GPU beside the token-rows pass on the same ids
(bert_hip_eval_packed_tokens_device, f16 rows, no embeddings): what the MLM transform and the vocabulary launch cost; and the vocabulary
launch alone (the profile's "sparse_vocab" + "sparse_finish" lines) beside torch's f16 matmul + segmented amax + log1p(relu) on rows of
the same shape.  minilm-l6 dims (V = 30 522), f16 file, two shapes: 256 sentences of 128 tokens and 4096 of 25.

    python tools/sparse_rate.py [--iters 10] [--rounds 5] [--out profiles/sparse_rate.txt]

Everything is in device memory; a figure is the time per call from device events around `iters` back-to-back calls on one stream (a
synchronise behind them), the median of `rounds` rounds, the calls alternating round by round after warm-up calls."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_rate.py needs a GPU")
    os.environ.setdefault("BERT_HIP_QUIET", "1")
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert

    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mlm.bin")
        hp = gf.MODEL_DIMS["minilm-l6"]
        gf.write_model(path, hp, gf.synthetic_weights(hp, 0, mlm_head=True), gf.FTYPE_F16)
        m = pybert.BertModel(path)
        dev = torch.device("cuda")
        stream = torch.cuda.current_stream().cuda_stream
        H, V = hp.n_embd, hp.n_vocab
        out(f"# bert_hip_sparse_packed_device beside bert_hip_eval_packed_tokens_device on the same ids, {torch.cuda.get_device_name(0)}; minilm-l6 dims, f16, "
            f"V = {V}; ms per call = median of {a.rounds} rounds of {a.iters} calls between device events, the calls alternating")
        for B, L in ((256, 128), (4096, 25)):
            T = B * L
            ids = gf.synthetic_token_ids(B, L, V, seed=3)
            d_ids = torch.from_numpy(ids.reshape(-1)).to(dev)
            d_cu = (torch.arange(0, B + 1, dtype=torch.int32) * L).to(dev)
            d_rows = torch.empty(T, H, dtype=torch.float16, device=dev)
            d_w = torch.empty(B, V, dtype=torch.float32, device=dev)
            m.reserve(T, B)

            def sparse():
                m.sparse_packed_device(d_ids.data_ptr(), d_cu.data_ptr(), B, T, L, d_w.data_ptr(), stream=stream)

            def tokens():
                m.eval_packed_tokens_device(d_ids.data_ptr(), d_cu.data_ptr(), B, T, L, d_rows.data_ptr(), None, False, True, stream)

            # torch on rows of the same shape: the pass's own f16 token rows stand in for t, a random f16 matrix for the vocabulary
            E = torch.randn(V, H, device=dev).half()
            bias = torch.randn(V, device=dev)

            def torch_head():
                return torch.log1p(torch.relu((d_rows @ E.T).view(B, L, V).amax(dim=1).float() + bias))

            for _ in range(2):
                sparse(); tokens(); torch_head()
            torch.cuda.synchronize()
            assert m.check() == 0 and bool(torch.isfinite(d_w).all()) and bool((d_w >= 0).all())
            zero = float((d_w == 0).float().mean())
            t_s, t_t, t_h = [], [], []
            for _ in range(a.rounds):
                t_s.append(timed(sparse)); t_t.append(timed(tokens)); t_h.append(timed(torch_head))
            m.profile(True)
            sparse()
            torch.cuda.synchronize()
            rep = m.profile_report()
            m.profile(False)
            one = lambda n: rep[n]["total_ms"] / max(rep[n]["launches"], 1) if n in rep else float("nan")
            ms, mt, mh = (float(np.median(x)) for x in (t_s, t_t, t_h))
            vocab_ms = one("sparse_vocab") + one("sparse_finish")
            flop = 2.0 * T * V * H
            out(f"# {B} sentences of {L} tokens ({T} tokens; the projection is {flop / 1e12:.3f} TFLOP; {zero:.2f} of the weights are zero)")
            out("# call                                ms (min .. max)     sentences/s")
            out(f"  sparse_packed_device        {ms:9.3f} ({min(t_s):.3f} .. {max(t_s):.3f}) {B / ms * 1e3:12.0f}")
            out(f"  eval_packed_tokens_device   {mt:9.3f} ({min(t_t):.3f} .. {max(t_t):.3f}) {B / mt * 1e3:12.0f}")
            out(f"  head (transform + vocabulary): {ms - mt:+.3f} ms per call; profiled alone: mlm_transform {one('mlm_transform') * 1e3:.1f} us, mlm_layernorm "
                f"{one('mlm_layernorm') * 1e3:.1f} us, sparse_vocab {one('sparse_vocab') * 1e3:.1f} us ({flop / one('sparse_vocab') / 1e9:.1f} TFLOP/s), "
                f"sparse_finish {one('sparse_finish') * 1e3:.1f} us")
            out(f"  vocabulary launch + finish {vocab_ms:.3f} ms beside torch f16 matmul + amax + log1p(relu) {mh:.3f} ms ({min(t_h):.3f} .. {max(t_h):.3f}): "
                f"{mh / vocab_ms:.2f} x; atomics: one 4-byte integer max per positive (sentence-in-tile, v), at most {B * V * 4 / 1e6:.0f} MB")
            del E, d_w, d_rows
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
