"""The int8 index's surface without a GPU: bert-search offers --i8, and the binding names the new dtype."""
import os
import subprocess

import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_example_usage_names_i8():
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    usage = [line for line in r.stderr.splitlines() if line.startswith("usage:")]
    assert usage and "--i8" in usage[0], r.stderr


def test_index_dtype_strings(sparse_vocab_model):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        with pytest.raises(ValueError, match="'i8'"):
            m.index(dtype="int4")
        # "i8" passes the binding's check and reaches bert_hip_index_create, which refuses a context without a device
        with pytest.raises(RuntimeError, match="bert_hip_index_create"):
            m.index(dtype="i8")
    finally:
        m.close()
