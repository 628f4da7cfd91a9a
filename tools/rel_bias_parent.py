#!/usr/bin/env python3
"""What tests/test_gpu_rel_bias.py and tests/test_gpu_rel_bias_edges.py hold the relative position bias to, measured on the PARENT
commit's library: the error of a model WITHOUT the tensor against the float64 model with W = 0 (the tests allow a model with the tensor
twice that) for rel_bias_reference.E2E_MODELS and E2E_EDGE_MODELS, and the digests of eval_packed on two BERT files (the test demands
the same bits).  Needs an MI355X.

    python tools/rel_bias_parent.py --parent DIR

DIR: bert.cpp_amd of a built checkout of the parent commit (its pybert.py and libbert.so).  The model files, sentences and the float64
model are this checkout's (tests/rel_bias_reference.py): the same ones the tests use.  Prints the dictionaries to paste into the test."""
import argparse
import hashlib
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("BERT_HIP_QUIET", "1")
os.environ.setdefault("BERT_HIP_LATENCY", "128")          # (as tests/conftest.py sets it)

import rel_bias_reference as rb          # noqa: E402
import test_gpu_rel_bias as T            # noqa: E402
import test_gpu_rel_bias_edges as TE     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("pybert_parent", os.path.join(a.parent, "pybert.py"))
    pb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pb)
    print("library:", pb.LIB_PATH, pb.lib().bert_hip_version().decode())
    pooled, hidden, bits = {}, {}, {}
    with tempfile.TemporaryDirectory() as d:
        for name in rb.E2E_MODELS:
            path = T.e2e_file(d, name, rel_bias=False)
            ref = rb.Model(path, use_bias=False)
            m = pb.BertModel(path)
            sents = rb.e2e_sentences(name)
            got = m.eval_packed(np.concatenate(sents), rb.cu_of([len(s) for s in sents]))
            hid = [ref.hidden(s) for s in sents]
            want = np.stack([h[-1].mean(axis=0) / np.linalg.norm(h[-1].mean(axis=0)) for h in hid])
            pooled[name] = rb.row_error(got, want)
            per = [rb.row_error(m.eval_hidden(s)[1], h) for s, h in zip(sents, hid)]
            hidden[name] = max(per)
            print(f"{name}: pooled {pooled[name]:.3e}; hidden per length " + " ".join(f"{len(s)}:{e:.2e}" for s, e in zip(sents, per)))
            m.close()
        edge_pooled, edge_hidden = {}, {}
        for name in rb.E2E_EDGE_MODELS:
            path = TE.edge_file(d, name, rel_bias=False)
            m = pb.BertModel(path)
            edge_pooled[name], per, _ = TE.edge_errors(m, rb.Model(path, use_bias=False), rb.edge_calls(name))
            edge_hidden[name] = float(np.max(list(per.values())))
            print(f"{name}: pooled {edge_pooled[name]:.3e}; hidden per length " + " ".join(f"{n}:{e:.2e}" for n, e in per.items()))
            m.close()
        for which in T.PARENT_BITS:
            path, toks, cu = T.bits_case(d, which)
            m = pb.BertModel(path)
            m.profile(True)
            out = m.eval_packed(toks, cu)
            print(which, "launches", {k: v["launches"] for k, v in m.profile_report().items()})
            m.profile(False)
            bits[which] = hashlib.sha256(m.eval_packed(toks, cu).tobytes()).hexdigest()
            assert np.array_equal(out, m.eval_packed(toks, cu))
            m.close()
    fmt = lambda d: "{" + ", ".join(f'"{k}": {v:.3e}' for k, v in d.items()) + "}"
    print("PARENT_POOLED_ERROR =", fmt(pooled))
    print("PARENT_HIDDEN_ERROR =", fmt(hidden))
    print("PARENT_BITS =", bits)
    print("tests/test_gpu_rel_bias_edges.py:")
    print("PARENT_POOLED_ERROR =", fmt(edge_pooled))
    print("PARENT_HIDDEN_ERROR =", fmt(edge_hidden))


if __name__ == "__main__":
    main()
