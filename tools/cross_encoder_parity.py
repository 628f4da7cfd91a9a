#!/usr/bin/env python3
"""What an UNTYPED pass leaves between the device and a float64 model on the batches of tests/test_gpu_cross_encoder.py's end-to-end test:
per model, the worst |row - float64| / max |row| of the un-normalised [CLS] rows of bert_hip_eval_packed (pooling cls, normalize 0; token
type 0 everywhere).  Run on the commit BEFORE token types (BERT_HIP_LIB = that commit's libbert.so; it needs nothing newer than
bert_hip_eval_packed), the figures are the basis of the typed test's tolerance: profiles/cross_encoder_parity.txt.

usage: python tools/cross_encoder_parity.py [OUT.txt]          (needs a GPU)"""
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
import cross_encoder_reference as cer  # noqa: E402

# (bound by hand, not through pybert: an older library lacks symbols pybert declares)
LIB_PATH = os.environ.get("BERT_HIP_LIB") or os.path.join(ROOT, "bert.cpp_amd", "libbert.so")


def main(out_path):
    L = C.CDLL(LIB_PATH)
    vp, i32p = C.c_void_p, C.POINTER(C.c_int32)
    L.bert_load_from_file.restype = vp; L.bert_load_from_file.argtypes = [C.c_char_p]
    L.bert_free.restype = None; L.bert_free.argtypes = [vp]
    L.bert_hip_set_option.restype = None; L.bert_hip_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.bert_hip_eval_packed.restype = C.c_int32; L.bert_hip_eval_packed.argtypes = [vp, i32p, i32p, C.c_int32, C.POINTER(C.c_float)]
    L.bert_hip_version.restype = C.c_char_p
    lines = ["# worst |row - float64| / max |row| of bert_hip_eval_packed's un-normalised [CLS] rows (pooling cls, normalize 0, token type 0),",
             "# per model over the batches of tests/cross_encoder_reference.py e2e_batches", f"# {L.bert_hip_version().decode()}",
             "# dims ftype batch worst"]
    with tempfile.TemporaryDirectory() as d:
        for dims, ftype in cer.E2E_MODELS:
            path = os.path.join(d, f"{dims}_{ftype}.bin")
            hp = cer.DIMS[dims]
            gf.write_model(path, hp, gf.synthetic_weights(hp, cer.E2E_SEED), gf.FTYPE_BY_NAME[ftype])       # (no head: the same encoder)
            ref = cer.Model(path)
            ctx = L.bert_load_from_file(path.encode())
            assert ctx, path
            L.bert_hip_set_option(ctx, b"pooling", b"cls"); L.bert_hip_set_option(ctx, b"normalize", b"0")
            worst = 0.0
            for name, (toks, cu, _, sents) in cer.e2e_batches(dims).items():
                rows32 = np.full((len(sents), hp.n_embd), np.nan, dtype=np.float32)
                r = L.bert_hip_eval_packed(ctx, toks.ctypes.data_as(i32p), cu.ctypes.data_as(i32p), len(sents), rows32.ctypes.data_as(C.POINTER(C.c_float)))
                assert r == 0, r
                rows = rows32.astype(np.float64)
                want = np.stack([ref.cls_row(s) for s in sents])
                err = float((np.abs(rows - want) / np.abs(want).max(axis=1, keepdims=True)).max())
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
