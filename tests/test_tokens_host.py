"""Token rows and MaxSim without a GPU: the new names in the symbol lists, the headers and the libraries; a tokenizer-only context is
refused; the reference's bound (maxsim_reference.py) holds for a NumPy f32 restatement of the chain, so it can be met."""
import os
import re
import subprocess

import numpy as np
import pytest

import maxsim_reference as mr
from bert_cpp_amd import pybert

from conftest import ROOT

NEW = ["bert_hip_eval_packed_tokens_device", "bert_hip_eval_packed_tokens", "bert_hip_encode_tokens_batch", "bert_hip_maxsim_device", "bert_hip_maxsim"]


def test_header_lists_and_libraries_hold_the_new_names():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    assert "TOKEN ROWS AND LATE INTERACTION" in text
    for sym in NEW:
        assert re.search(r"BERT_API\s+int(32|64)_t\s+%s\s*\(\s*struct bert_ctx\s*\*" % sym, text), sym
        assert sym in pybert.BERT_HIP_H_SYMBOLS
    # libbert.map exports bert_* and nothing else: the names are in both libraries, the test hook in the test library only
    exported = {p: subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout.split() for p in (pybert.LIB_PATH, pybert.TEST_LIB_PATH)}
    for sym in NEW:
        assert sym in exported[pybert.LIB_PATH] and sym in exported[pybert.TEST_LIB_PATH], sym
    assert "global: bert_*;" in open(os.path.join(ROOT, "bert.cpp_amd", "libbert.map")).read()
    test_h = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    assert re.search(r"BERT_API\s+int32_t\s+bert_hip_test_token_rows\s*\(", test_h) and "bert_hip_test_token_rows" in pybert.BERT_HIP_TEST_H_SYMBOLS
    assert "bert_hip_test_token_rows" in exported[pybert.TEST_LIB_PATH] and "bert_hip_test_token_rows" not in exported[pybert.LIB_PATH]
    for name in ("eval_packed_tokens", "eval_packed_tokens_device", "encode_tokens", "maxsim", "maxsim_device"):
        assert callable(getattr(pybert.BertModel, name)), name
    assert callable(pybert.test_token_rows)


def test_a_tokenizer_only_context_is_refused(sparse_vocab_model):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    L, vp = m.lib, None
    toks = np.array([101, 102], dtype=np.int32); cu = np.array([0, 2], dtype=np.int32)
    rows = np.full((2, m.n_embd), 7.0, dtype=np.float32)
    sc = np.full(1, 7.0, dtype=np.float32)
    i32p, f32p = pybert._i32p, pybert._f32p
    assert L.bert_hip_eval_packed_tokens(m.ctx, i32p(toks), i32p(cu), 1, 1, f32p(rows), None) == -1
    assert L.bert_hip_eval_packed_tokens_device(m.ctx, vp, vp, 1, 2, 2, 1, vp, vp, vp) == -1
    txt = (pybert.C.c_char_p * 1)(b"hello")
    assert L.bert_hip_encode_tokens_batch(m.ctx, 1, 1, txt, 1, i32p(cu), None, 0) == -1
    assert L.bert_hip_maxsim(m.ctx, f32p(rows), i32p(cu), 1, f32p(rows), i32p(cu), 1, 8, None, 0, 0, f32p(sc)) == -1
    assert L.bert_hip_maxsim_device(m.ctx, vp, vp, 1, vp, vp, 1, 8, vp, 0, 0, vp, vp) == -1
    assert (rows == 7.0).all() and sc[0] == 7.0
    m.close()


@pytest.mark.parametrize("H", [8, 24, 64, 384])
def test_the_bound_holds_for_an_f32_restatement(H):
    """unit rows, and the all-negative set: the float64 score and the f32 restatement agree within the derived bound, sum and mean"""
    rng = np.random.default_rng(H)
    q, qcu, _ = mr.packed_set(rng, [1, 31, 33], H)
    d, dcu, _ = mr.packed_set(rng, [1, 32, 65], H)
    sets = [(q, qcu, d, dcu), mr.negative_sets(rng, [1, 33], [2, 40], H)]
    for q, qcu, d, dcu in sets:
        q16, d16 = mr.round_f16(q), mr.round_f16(d)
        for mean in (False, True):
            want, bound = mr.maxsim_reference(q16, qcu, d16, dcu, None, mean)
            got = mr.maxsim_f32(q16, qcu, d16, dcu, None, mean)
            frac = float((np.abs(got - want) / bound).max())
            print(f"H {H} mean {mean}: worst fraction of the bound {frac:.3f}")
            assert (bound > 0).all() and frac <= 1.0
    assert (mr.maxsim_reference(mr.round_f16(sets[1][0]), sets[1][1], mr.round_f16(sets[1][2]), sets[1][3])[0] < -0.5).all()


def test_the_token_row_bound_holds_for_an_f32_restatement():
    rng = np.random.default_rng(3)
    for H in (8, 130, 768):
        x = rng.normal(0.1, 1, (5, H)).astype(np.float16)
        x32 = x.astype(np.float32)
        sq = np.zeros(5, dtype=np.float32)
        for e in range(H):
            sq = sq + x32[:, e] * x32[:, e]
        got = x32 * (np.float32(1) / np.sqrt(sq))[:, None]
        for f16_out in (False, True):
            want, bound = mr.token_rows_reference(x, True, f16_out)
            g = got.astype(np.float16) if f16_out else got
            assert (np.abs(g.astype(np.float64) - want) <= bound).all(), (H, f16_out)
        want, bound = mr.token_rows_reference(x, False, False)
        assert (bound == 0).all() and np.array_equal(want, x32.astype(np.float64))
