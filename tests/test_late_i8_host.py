"""The token index's int8 form (include/bert_hip.h "TOKEN INDEX, int8 form") without a GPU: the three new symbols and the binding,
that no new exported name contains token_index, what the new entry points answer without an index or a device, bert-search's usage
errors, and the self-checks of the reference the GPU tests hold the kernels against (token_i8_reference.py)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

import token_i8_reference as t8
from conftest import ROOT
from test_late_index_host import TOKEN_INDEX_NAMES

NEW_SYMBOLS = ["bert_hip_late_index_create", "bert_hip_late_index_dtype", "bert_hip_late_index_get_codes"]
EXE = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")


# ------------------------------------------------------------------------------------------------
# symbols and the binding
# ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    exported = {p: subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout.split()
                for p in (pybert.LIB_PATH, pybert.TEST_LIB_PATH)}
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pybert.BERT_HIP_H_SYMBOLS, sym
        assert sym in exported[pybert.LIB_PATH] and sym in exported[pybert.TEST_LIB_PATH], sym
        assert "token_index" not in sym
    # the exported names that contain token_index are still the closed set
    for p in exported:
        assert sorted(s for s in exported[p] if "token_index" in s) == sorted(n for n in TOKEN_INDEX_NAMES if n in exported[p]), p
    assert "TOKEN INDEX, int8 form" in text and "(dpad + 4) / (2 dim)" in text
    L = pybert.lib()
    assert L.bert_hip_late_index_create.restype is C.c_void_p and len(L.bert_hip_late_index_create.argtypes) == 3


def test_binding_has_the_new_names_with_todays_defaults():
    sig = inspect.signature(pybert.BertModel.token_index)
    assert list(sig.parameters) == ["self", "dim", "dtype"] and sig.parameters["dim"].default is None and sig.parameters["dtype"].default == "f16"
    assert callable(pybert.BertTokenIndex.get_codes)
    assert inspect.signature(pybert.BertTokenIndex.__init__).parameters["dtype"].default == "f16"


# ------------------------------------------------------------------------------------------------
# refusals that need no device
# ------------------------------------------------------------------------------------------------
def test_entry_points_answer_minus_one_or_null_without_an_index(capfd):
    L = pybert.lib()
    codes = np.full((2, 32), 7, np.int8)
    scales = np.full(2, 7.0, np.float32)
    capfd.readouterr()
    assert L.bert_hip_late_index_dtype(None) == -1                      # (like size: no line)
    assert capfd.readouterr().err == ""
    assert L.bert_hip_late_index_get_codes(None, 0, codes.ctypes.data, scales.ctypes.data, 2) == -1
    assert "bert_hip_late_index_get_codes: no index" in capfd.readouterr().err
    for dtype in (1, 2, 0, 3):
        assert not L.bert_hip_late_index_create(None, 8, dtype)
        assert "bert_hip_late_index_create: no context" in capfd.readouterr().err
    assert (codes == 7).all() and (scales == 7.0).all()


def test_tokenizer_only_context_makes_no_int8_index(sparse_vocab_model, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        capfd.readouterr()
        assert not m.lib.bert_hip_late_index_create(m.ctx, 8, 2)
        assert "tokenizer-only" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            m.token_index(8, "i8")
        with pytest.raises(ValueError):
            m.token_index(8, "i4")
    finally:
        m.close()


def test_bert_search_names_the_flag_and_refuses_it_beside_the_file_flags(tmp_path):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--late [--i8]" in r.stderr and "bert_hip_late_index_create" in r.stderr
    f = tmp_path / "lines.txt"
    f.write_text("a\nb\n")
    base = [EXE, "-m", "nonexistent.bin", "-f", str(f)]
    for extra in (["--late", "--i8", "--save-tokens", "x"], ["--late", "--i8", "--load-tokens", "x"],
                  ["--maxsim", "5", "--token-index", "--i8", "--save-tokens", "x"], ["--i8", "--maxsim", "5", "--token-index", "--load-tokens", "x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--i8 with a token index does not go with --save-tokens or --load-tokens" in r.stderr, (extra, r.stderr)
    # without a file flag, --i8 beside a token index passes the argument checks: the run fails at the model file instead
    for extra in (["--late", "--i8"], ["--maxsim", "5", "--token-index", "--i8"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, 2), (extra, r.returncode, r.stderr)
    # --late still refuses the other stored types
    for flag in ("--f32", "--b1"):
        r = subprocess.run(base + ["--late", flag], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--late" in r.stderr, flag
    assert not (tmp_path / "x").exists()


# ------------------------------------------------------------------------------------------------
# the reference's self-checks
# ------------------------------------------------------------------------------------------------
def test_quantise_a_zero_row_and_the_padding():
    codes, scales = t8.quantise(np.zeros((2, 40), np.float32))
    assert codes.shape == (2, 64) and codes.dtype == np.int8 and not codes.any() and (scales == 0).all() and scales.dtype == np.float32
    rows = np.random.default_rng(0).standard_normal((3, 24)).astype(np.float32)
    codes, scales = t8.quantise(rows)
    assert codes.shape == (3, 32) and not codes[:, 24:].any() and (np.abs(codes).max(axis=1) == 127).all()
    assert [t8.dpad(d) for d in (8, 24, 32, 40, 128, 384, 1024)] == [32, 32, 32, 64, 128, 384, 1024]


def test_quantise_an_exactly_representable_scale():
    """amax 127 gives scale 1: the codes are the roundings of the elements themselves"""
    row = np.array([[127.0, -127.0, 3.0, -0.0, 1.25, -64.75, 0.49, 126.6]], np.float32)
    codes, scales = t8.quantise(row)
    assert scales[0] == 1.0 and codes[0, :8].tolist() == [127, -127, 3, 0, 1, -65, 0, 127]
    # amax 63.5 gives scale 0.5
    codes, scales = t8.quantise(np.array([[63.5, 1.0, -0.25, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32))
    assert scales[0] == 0.5 and codes[0, :3].tolist() == [127, 2, 0]


def test_quantise_rounds_halves_to_even():
    """scale 1: x.5 lies exactly between two codes and goes to the even one"""
    row = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5]], np.float32)
    codes, _ = t8.quantise(row)
    assert codes[0, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 126]


def test_quantise_non_finite_rows():
    rows = np.ones((4, 8), np.float32)
    rows[0, 3], rows[1, 0], rows[2, 7] = np.nan, np.inf, -np.inf
    codes, scales = t8.quantise(rows)
    assert np.isnan(scales[:3]).all() and not codes[:3].any()
    assert scales[3] == np.float32(1.0) / np.float32(127.0) and (codes[3, :8] == 127).all()
    # large finite rows stay finite
    codes, scales = t8.quantise(np.full((1, 8), 6e4, np.float32))
    assert np.isfinite(scales[0]) and (codes[0, :8] == 127).all()


def test_the_butterfly_sum_against_an_explicit_pairing():
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(32) * 10.0 ** rng.integers(-3, 4, 32)).astype(np.float32)
    f = np.float32
    # lane 0 after lane ^ 32 (+0), ^ 16, ^ 8, ^ 4, ^ 2, ^ 1, written out: at every level lane l holds its own value plus lane l ^ o's
    lvl = [f(x + f(0)) for x in v]
    for o in (16, 8, 4, 2, 1):
        lvl = [f(lvl[l] + lvl[l ^ o]) for l in range(32)]
    assert t8.butterfly_sum(v).view(np.uint32) == lvl[0].view(np.uint32)
    assert len({x.view(np.uint32).item() for x in lvl}) == 1            # every lane holds the same bits: addition is commutative
    # it is not the left-to-right sum for these values
    seq = f(0)
    for x in v:
        seq = f(seq + x)
    assert abs(float(t8.butterfly_sum(v)) - float(v.astype(np.float64).sum())) < 1e-2 and seq.dtype == np.float32
    # columns are independent
    m = rng.standard_normal((32, 5)).astype(np.float32)
    assert all(t8.butterfly_sum(m)[c].view(np.uint32) == t8.butterfly_sum(m[:, c]).view(np.uint32) for c in range(5))


def test_scores_i8_on_a_case_worked_by_hand():
    """dim 8, scale 1 rows: the score is the sum over the query's tokens of the largest integer inner product"""
    e = lambda i, v=127.0: np.eye(8, dtype=np.float32)[i] * np.float32(v)
    q = np.stack([e(0), e(1) + e(0, 2.0)])                               # two tokens, both of amax 127: scale 1
    d = np.stack([e(0), e(1), e(2), e(0, -127.0)])                       # documents [0, 1], [2], [3]
    dcu = np.array([0, 2, 3, 4], np.int32)
    S = t8.scores_i8(q, [0, 2], d, dcu)
    assert S.dtype == np.float32 and S.shape == (1, 3)
    assert S[0].tolist() == [127.0 * 127 + 127.0 * 127, 0.0, -127.0 * 127 - 2 * 127.0]
    f64, bound = t8.scores_f64(q, [0, 2], d, dcu)
    assert (np.abs(S - f64) <= bound).all() and (bound < 0.05 * np.abs(f64).max()).all()
    # a NaN token in a document, and in the query
    d2 = d.copy()
    d2[2, 5] = np.nan
    S2 = t8.scores_i8(q, [0, 2], d2, dcu)
    assert np.isnan(S2[0, 1]) and S2[0, 0] == S[0, 0] and S2[0, 2] == S[0, 2]
    q2 = np.concatenate([q, q])
    q2[3, 0] = np.inf
    S3 = t8.scores_i8(q2, [0, 2, 4], d, dcu)
    assert np.array_equal(S3[0], S[0]) and np.isnan(S3[1]).all()


def test_scores_i8_does_not_depend_on_the_neighbours_or_the_offsets():
    rng = np.random.default_rng(4)
    q = rng.standard_normal((70, 24)).astype(np.float32)
    d = rng.standard_normal((90, 24)).astype(np.float32)
    qcu, dcu = np.array([0, 33, 34, 70], np.int32), np.array([0, 1, 40, 41, 90], np.int32)
    S = t8.scores_i8(q, qcu, d, dcu)
    assert np.isfinite(S).all()
    alone = t8.scores_i8(q[33:34], [0, 1], d[1:40], [0, 39])
    assert alone.view(np.uint32)[0, 0] == S.view(np.uint32)[1, 1]
    f64, bound = t8.scores_f64(q, qcu, d, dcu)
    assert (np.abs(S - f64) <= bound).all()
