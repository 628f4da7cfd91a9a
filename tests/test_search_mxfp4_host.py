"""The MXFP4 index form (dtype 4, "mxfp4") without a GPU: the binding's dtype name and bert-search's option."""
import os
import subprocess

import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mxfp4_is_a_dtype_of_the_binding_and_an_option_of_the_example(sparse_vocab_model, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        capfd.readouterr()
        # the name is accepted and the call reaches bert_hip_index_create, which refuses a context without a device
        with pytest.raises(RuntimeError, match="bert_hip_index_create"):
            m.index(dtype="mxfp4")
        assert "bert_hip_index_create" in capfd.readouterr().err
        with pytest.raises(ValueError, match="'i8'.*'b1'.*'mxfp4'"):
            m.index(dtype="mxfp8")
    finally:
        m.close()
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search"), "-h"], capture_output=True, text=True, timeout=60)
    usage = [line for line in r.stderr.splitlines() if line.startswith("usage:")]
    assert r.returncode == 0 and usage and all(opt in usage[0] for opt in ("--mxfp4", "--b1", "--rescore", "--i8", "--save", "--load")), r.stderr
