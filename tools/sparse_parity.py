#!/usr/bin/env python3
"""What a token-rows pass leaves between the device and a float64 model on the batches of tests/test_gpu_sparse.py's end-to-end test: per
model, the worst |state - float64| / max |state of that token| of bert_hip_eval_packed_tokens' un-normalised rows (flags 0).  Run on the
commit BEFORE the MLM head (BERT_HIP_LIB = that commit's libbert.so; it needs nothing newer than bert_hip_eval_packed_tokens, and the
models are written without the head: a seed gives the same encoder), the figures are the basis of the sparse test's `drows`:
profiles/sparse_parity.txt.

usage: python tools/sparse_parity.py [OUT.txt]          (needs a GPU)"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("BERT_HIP_QUIET", "1")
os.environ.setdefault("BERT_HIP_LATENCY", "128")               # (the test suite's setting: tests/conftest.py)

from bert_cpp_amd import ggml_file as gf  # noqa: E402
import sparse_reference as sr  # noqa: E402

# (bound by hand, not through pybert: an older library lacks symbols pybert declares)
LIB_PATH = os.environ.get("BERT_HIP_LIB") or os.path.join(ROOT, "bert.cpp_amd", "libbert.so")


def main(out_path):
    L = C.CDLL(LIB_PATH)
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    L.bert_load_from_file.restype = vp; L.bert_load_from_file.argtypes = [C.c_char_p]
    L.bert_free.restype = None; L.bert_free.argtypes = [vp]
    L.bert_hip_eval_packed_tokens.restype = C.c_int32; L.bert_hip_eval_packed_tokens.argtypes = [vp, i32p, i32p, C.c_int32, C.c_int32, f32p, f32p]
    L.bert_hip_version.restype = C.c_char_p
    has_head = hasattr(L, "bert_hip_has_mlm_head")
    lines = ["# worst |state - float64| / max |state of the token| of bert_hip_eval_packed_tokens' un-normalised rows (flags 0),",
             "# per model over the batches of tests/sparse_reference.py e2e_batches",
             f"# {L.bert_hip_version().decode()}; the library {'has' if has_head else 'does not have'} bert_hip_has_mlm_head", "# dims ftype batch worst"]
    with tempfile.TemporaryDirectory() as d:
        for dims, ftype in sr.E2E_MODELS:
            path = os.path.join(d, f"{dims}_{ftype}.bin")
            hp = sr.DIMS[dims]
            gf.write_model(path, hp, sr.model_weights(dims, mlm_head=False), gf.FTYPE_BY_NAME[ftype])       # (no head: the same encoder)
            ref = sr.Model(path)
            ctx = L.bert_load_from_file(path.encode())
            assert ctx, path
            worst = 0.0
            for name, (toks, cu, sents) in sr.e2e_batches(dims).items():
                rows32 = np.full((len(toks), hp.n_embd), np.nan, dtype=np.float32)
                r = L.bert_hip_eval_packed_tokens(ctx, toks.ctypes.data_as(i32p), cu.ctypes.data_as(i32p), len(sents), 0, rows32.ctypes.data_as(f32p), None)
                assert r == 0, r
                want = np.concatenate([ref.states(s) for s in sents])
                err = float((np.abs(rows32.astype(np.float64) - want) / np.abs(want).max(axis=1, keepdims=True)).max())
                lines.append(f"{dims} {ftype} {name} {err:.3e}")
                worst = max(worst, err)
            lines.append(f"{dims} {ftype} ALL {worst:.3e}")
            L.bert_free(ctx)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
