"""The pooling settings of a context (include/bert_hip.h: "pooling" / "normalize") where no GPU is needed: the header declares the
two getters, the product library exports them, and a context without a device answers -1 and takes the keys as no-ops."""
import ctypes as C
import os
import re
import subprocess

from bert_cpp_amd import pybert

from conftest import ROOT

GETTERS = ("bert_hip_pooling", "bert_hip_normalize")


def test_header_declares_and_library_exports_the_getters():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    for sym in GETTERS:
        assert re.search(r"BERT_API\s+int32_t\s+%s\s*\(\s*struct bert_ctx\s*\*" % sym, text), sym
        assert sym in pybert.BERT_HIP_H_SYMBOLS
    names = subprocess.run(["nm", "-D", "--defined-only", pybert.LIB_PATH], capture_output=True, text=True).stdout.split()
    for sym in GETTERS:
        assert sym in names, sym
    # the header describes both settings where it describes the environment
    for word in ("BERT_HIP_POOLING", "BERT_HIP_NORMALIZE", '"pooling"', '"normalize"'):
        assert word in text, word


def test_context_without_a_device_answers_minus_one(sparse_vocab_model):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    assert m.pooling() == -1 and m.normalize() == -1
    L = pybert.lib()
    assert L.bert_hip_pooling(None) == -1 and L.bert_hip_normalize(None) == -1


def test_keys_are_harmless_on_a_tokenizer_only_context(sparse_vocab_model, tok_golden):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    t = tok_golden["tests"][0]
    before = m.tokenize(t["text"])
    m.set_option("pooling", "cls")
    m.set_option("normalize", "0")
    m.set_option("pooling", "max")
    assert m.pooling() == -1 and m.normalize() == -1
    assert m.tokenize(t["text"]) == before == t["ids"]


def test_the_test_hook_is_bound_and_stays_out_of_the_product_library():
    assert "bert_hip_test_pool" in pybert.BERT_HIP_TEST_H_SYMBOLS
    T = pybert.test_lib()
    assert T.bert_hip_test_pool.argtypes[5:7] == [C.c_int32, C.c_int32]
    assert not hasattr(pybert.lib(), "bert_hip_test_pool")
