"""The MXFP8 weight image's host packer (weights.cpp pack_mx_image through bert_hip_test_pack_mx) against mxfp4_reference.mxfp8_queries,
the two hooks' places in the headers and libraries, and the BERT_HIP_MX switch's report of a value it does not know.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert
from conftest import ROOT
from mxfp4_reference import mxfp8_queries

HOOKS = ["bert_hip_test_pack_mx", "bert_hip_test_gemm_mx"]


def weights(N, K):
    """f16 [N, K]: plain blocks; row 1 starts with a zero block, row 2 with a block whose maximum is a power of two, and row 3 ends with
    a block whose maximum 1.99 scales to 509: the outlier clamps at 448"""
    w = (np.random.default_rng(N + K).standard_normal((N, K)) * 0.05).astype(np.float16)
    w[1, 0:32] = 0
    w[2, 0:32] = np.float16(0.25) * np.sign(w[2, 0:32].astype(np.float32) + 1e-9) * (np.arange(32) % 4 == 0)
    w[3, K - 32:K] = np.float16(0.01)
    w[3, K - 1] = np.float16(1.99)
    return w


@pytest.mark.parametrize("N,K", [(128, 64), (384, 768)])
def test_packed_image_is_the_reference_rule_bit_for_bit(N, K):
    w = weights(N, K)
    codes, scales = pybert.test_pack_mx(w)
    want = mxfp8_queries(w.astype(np.float32))
    assert np.array_equal(pybert.mx_decode(codes, scales).view(np.int32) & 0x7fffffff, want.view(np.int32) & 0x7fffffff)
    assert np.array_equal(codes >> 7, np.signbit(w).astype(np.uint8))
    # the zero block: scale 2^0 and zero codes; the power of two 2^-2: e = -2 - 8; the clamp: 1.99 -> e = -8, code 0x7e = 448
    assert scales[1, 0] == 127 and not codes[1, 0:32].any()
    assert scales[2, 0] == 127 - 10 and set(codes[2, 0:32] & 0x7f) == {0, 0x78}
    assert scales[3, K // 32 - 1] == 127 - 8 and codes[3, K - 1] == 0x7e


def test_hooks_are_declared_listed_and_exported_by_the_test_library_only():
    with open(os.path.join(ROOT, "include", "bert_hip_test.h")) as f:
        test_h = f.read()
    with open(os.path.join(ROOT, "include", "bert_hip.h")) as f:
        product_h = f.read()
    nm = lambda lib: subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    test_syms, product_syms = nm(pybert.TEST_LIB_PATH), nm(pybert.LIB_PATH)
    for name in HOOKS:
        assert re.search(r"\b%s\(" % name, test_h) and name not in product_h
        assert name in pybert.BERT_HIP_TEST_H_SYMBOLS and name not in pybert.BERT_HIP_H_SYMBOLS
        assert re.search(r" T %s$" % name, test_syms, re.M) and name not in product_syms


def test_unknown_value_of_the_switch_is_reported_and_ignored(make_model, monkeypatch, capfd):
    # (the report comes before the load looks for a device: the same line with and without a GPU)
    path, _ = make_model("tiny-h128", "f16", 1)
    monkeypatch.setenv("BERT_HIP_MX", "fp4")
    try:
        m = pybert.BertModel(path)
    except RuntimeError:
        m = None                                              # (no GPU here)
    err = capfd.readouterr().err
    assert 'BERT_HIP_MX = "fp4"' in err and "ignored" in err
    if m is not None:
        m.set_option("mx", "1")                               # no images were built: refused
        assert "mx=1 needs BERT_HIP_MX=fp8" in capfd.readouterr().err
        m.close()
