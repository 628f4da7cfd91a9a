"""The token index's life cycle (include/bert_hip.h "LATE INDEX") without a GPU: the new symbols and the binding, that no new exported
name contains token_index, what every new entry point answers without an index or on a tokenizer-only context, the header and body
checks bert_hip_late_index_load runs (token_index_file.h through bert_hip_test_late_index_header / _body), make check-host, and
bert-search's two new flags."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

import token_index_file as tf
from conftest import ROOT

NEW_SYMBOLS = ["bert_hip_late_index_" + s for s in (
    "remove", "n_live", "n_live_tokens", "search_filtered", "search_filtered_device", "compact", "save", "load")]
HOOKS = ["bert_hip_test_late_index_header", "bert_hip_test_late_index_body"]
# the exported names that contain token_index: closed (tests/test_token_index_host.py)
TOKEN_INDEX_NAMES = ["bert_hip_token_index_" + s for s in (
    "create", "free", "size", "n_tokens", "max_query_tokens", "reserve", "add", "add_device", "add_texts", "get_doc", "search", "search_device",
    "search_texts", "rescore", "rescore_device")] + ["bert_hip_test_token_index_plan"]
EXE = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")


def check(buf, size):
    fields = (C.c_uint32 * 6)(*([0xFFFFFFFF] * 6))
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_late_index_header(buf, len(buf), size, fields, err, len(err))
    return r, list(fields), err.value.decode()


def check_body(fields, body):
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_late_index_body((C.c_uint32 * 6)(*fields), bytes(body), len(body), err, len(err))
    return r, err.value.decode()


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
    test_text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    for hook in HOOKS:
        assert re.search(r"BERT_API int32_t " + hook + r"\(", test_text) and hook in pybert.BERT_HIP_TEST_H_SYMBOLS and hook not in text
        assert hook in exported[pybert.TEST_LIB_PATH] and hook not in exported[pybert.LIB_PATH]
    # no exported name of either library outside the sixteen contains token_index
    for p in exported:
        assert sorted(s for s in exported[p] if "token_index" in s) == sorted(n for n in TOKEN_INDEX_NAMES if n in exported[p]), p
    assert sorted(s for s in exported[pybert.TEST_LIB_PATH] if "token_index" in s) == sorted(TOKEN_INDEX_NAMES)
    assert "LATE INDEX" in text and "BHIPTOK1" in text and "set of exported names that contain token_index is closed" in text
    assert pybert.lib().bert_hip_late_index_n_live_tokens.restype is C.c_int64


def test_binding_has_the_new_methods_with_todays_defaults():
    sig = inspect.signature(pybert.BertTokenIndex.search)
    assert sig.parameters["allow"].default is None and list(sig.parameters)[:4] == ["self", "q_rows", "q_cu", "k"]
    sig = inspect.signature(pybert.BertTokenIndex.search_device)
    assert sig.parameters["d_allow_ptr"].default is None and sig.parameters["n_words"].default == 0
    assert list(sig.parameters)[:9] == ["self", "n_queries", "d_qcu_ptr", "d_q_ptr", "max_q_len", "k", "d_ids_ptr", "d_scores_ptr", "stream"]
    for name in ("remove", "n_live", "n_live_tokens", "compact", "save", "live_ids"):
        assert callable(getattr(pybert.BertTokenIndex, name)), name
    assert callable(pybert.BertModel.load_token_index)


# ------------------------------------------------------------------------------------------------
# refusals that need no device
# ------------------------------------------------------------------------------------------------
def test_entry_points_answer_minus_one_without_an_index(tmp_path, capfd):
    L = pybert.lib()
    ids = np.full((1, 4), 7, np.int32)
    sc = np.full((1, 4), 7.0, np.float32)
    cu = np.array([0, 1], np.int32)
    rows = np.zeros((1, 8), np.float32)
    words = np.ones(1, np.uint32)
    p = lambda a: a.ctypes.data
    path = os.fsencode(str(tmp_path / "x.tok"))
    capfd.readouterr()
    assert L.bert_hip_late_index_n_live(None) == -1 and L.bert_hip_late_index_n_live_tokens(None) == -1     # (like size: no line)
    assert capfd.readouterr().err == ""
    assert L.bert_hip_late_index_remove(None, 1, p(ids)) == -1
    assert L.bert_hip_late_index_search_filtered(None, 1, p(cu), p(rows), 4, p(words), 1, p(ids), p(sc)) == -1
    assert L.bert_hip_late_index_search_filtered_device(None, 1, None, None, 32, 4, None, 0, None, None, None) == -1
    assert L.bert_hip_late_index_compact(None, p(ids)) == -1
    assert L.bert_hip_late_index_save(None, path) == -1
    err = capfd.readouterr().err
    for name in ("remove", "search_filtered", "search_filtered_device", "compact", "save"):
        assert f"bert_hip_late_index_{name}: no index" in err, name
    assert len(err.strip().splitlines()) == 5                            # one line each, nothing else
    assert not L.bert_hip_late_index_load(None, path)
    assert "bert_hip_late_index_load: no context" in capfd.readouterr().err
    assert (ids == 7).all() and (sc == 7.0).all() and (rows == 0).all()
    assert not (tmp_path / "x.tok").exists() and not (tmp_path / "x.tok.tmp").exists()


def test_tokenizer_only_context_loads_no_token_index(sparse_vocab_model, tmp_path, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        good = tmp_path / "empty.tok"
        good.write_bytes(tf.write(np.zeros((0, 8), np.float32), [0]))       # a valid file of an empty index
        assert check(good.read_bytes()[:64], 68)[0] == 0
        capfd.readouterr()
        assert not m.lib.bert_hip_late_index_load(m.ctx, os.fsencode(str(good)))
        assert "tokenizer-only" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            m.load_token_index(str(good))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n_docs,has_live,n_tokens", [
    (384, 1000, 1, 25000), (64, 33, 0, 40), (8, 0, 0, 0), (8, 0, 1, 0), (1024, 65, 1, 2 ** 31 - 2), (8, 1, 0, 1),
    # byte counts beyond 32 bits: 1.1 x 10^9 rows of 1024 halfs are past 2^41 bytes; the largest file needs 42 bits
    (1024, 1000, 0, 1100000000), (1024, 2 ** 31 - 1, 1, 2 ** 31 - 1)])
def test_good_headers_are_accepted(dim, n_docs, has_live, n_tokens):
    assert len(tf.header()) == 64
    size = tf.file_bytes(dim, n_docs, has_live, n_tokens)
    r, fields, err = check(tf.header(dim, n_docs, has_live, n_tokens), size)
    assert r == 0 and err == "", err
    assert fields == [1, dim, n_docs, has_live, n_tokens & 0xFFFFFFFF, n_tokens >> 32]


def test_file_length_arithmetic():
    assert tf.file_bytes(384, 1000, 1, 25000) == 64 + 1001 * 4 + 25000 * 768 + 32 * 4
    assert tf.file_bytes(8, 33, 0, 40) == 64 + 34 * 4 + 40 * 16
    assert tf.file_bytes(8, 0, 1, 0) == 68
    assert tf.file_bytes(1024, 1000, 0, 1100000000) > 2 ** 41
    big = tf.file_bytes(1024, 2 ** 31 - 1, 1, 2 ** 31 - 1)
    assert big == 64 + 2 ** 33 + (2 ** 31 - 1) * 2048 + 2 ** 28 and 2 ** 41 < big < 2 ** 43


def _bad_headers():
    good = tf.file_bytes(384, 1000, 1, 25000)
    yield "wrong magic", tf.header(magic=b"BHIPSPX1"), good
    yield "version 0", tf.header(version=0), good
    yield "version 2", tf.header(version=2), good
    for dim in (0, 12, 1032):
        yield f"dim {dim}", tf.header(dim=dim), tf.file_bytes(dim, 1000, 1, 25000)
    yield "n_tokens 2^31", tf.header(8, 1000, 0, 2 ** 31), tf.file_bytes(8, 1000, 0, 2 ** 31)
    yield "n_tokens 2^32 + 25000", tf.header(n_tokens=2 ** 32 + 25000), good
    yield "n_docs > n_tokens", tf.header(8, 41, 0, 40), tf.file_bytes(8, 41, 0, 40)
    yield "has_live 2", tf.header(has_live=2), good
    yield "first reserved byte", tf.header(reserved=b"\1" + b"\0" * 31), good
    yield "last reserved byte", tf.header(reserved=b"\0" * 31 + b"\1"), good
    yield "one byte short", tf.header(), good - 1
    yield "one byte long", tf.header(), good + 1
    yield "header only", tf.header(), 64
    yield "short buffer", tf.header()[:63], good
    yield "empty buffer", b"", good
    yield "length equal modulo 2^32", tf.header(1024, 1000, 0, 1100000000), tf.file_bytes(1024, 1000, 0, 1100000000) & 0xFFFFFFFF


@pytest.mark.parametrize("name,buf,size", list(_bad_headers()), ids=[c[0] for c in _bad_headers()])
def test_bad_headers_are_refused_with_a_reason(name, buf, size):
    r, fields, err = check(buf, size)
    assert r == -1 and err, name
    assert fields == [0xFFFFFFFF] * 6                                     # untouched
    L = pybert.test_lib()
    e = C.create_string_buffer(64)
    assert L.bert_hip_test_late_index_header(tf.header(), -1, 64, None, e, len(e)) == -1 and e.value
    assert L.bert_hip_test_late_index_header(tf.header(), 64, -1, None, e, len(e)) == -1 and e.value


# ------------------------------------------------------------------------------------------------
# the body
# ------------------------------------------------------------------------------------------------
def _body(n_docs=65, dim=8, has_live=1):
    """(fields, body as a bytearray, offset of the live words): document d has 1 + d % 3 tokens, every document live"""
    lens = [1 + d % 3 for d in range(n_docs)]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    data = tf.write(np.zeros((int(cu[-1]), dim), np.float32), cu, np.ones(n_docs, bool) if has_live else None)
    fields = [1, dim, n_docs, has_live, int(cu[-1]), 0]
    return fields, bytearray(data[64:]), (n_docs + 1) * 4 + int(cu[-1]) * dim * 2


def _set_cu(body, i, v):
    body[4 * i:4 * i + 4] = int(v & 0xFFFFFFFF).to_bytes(4, "little")


def _cu(body, i):
    return int.from_bytes(body[4 * i:4 * i + 4], "little")


def test_good_bodies_are_accepted():
    for n_docs, has_live in ((0, 0), (0, 1), (1, 1), (65, 0), (65, 1), (300, 1)):
        fields, body, _ = _body(n_docs, 8, has_live)
        assert check_body(fields, body) == (0, ""), (n_docs, has_live)
    # a removed last document of a full word
    fields, body, at = _body(64)
    body[-1] = 0x7F
    assert check_body(fields, body) == (0, "")
    # the rows are not looked at
    fields, body, at = _body(65)
    body[66 * 4:at] = b"\xff" * (at - 66 * 4)
    assert check_body(fields, body) == (0, "")


def _bad_bodies():
    def case(name, change):
        fields, body, at = _body()
        change(body, at)
        return name, fields, body
    yield case("cu[0] = 1", lambda b, at: _set_cu(b, 0, 1))
    yield case("cu[0] = -1", lambda b, at: _set_cu(b, 0, -1))
    yield case("an equal pair", lambda b, at: _set_cu(b, 7, _cu(b, 6)))
    yield case("a descent", lambda b, at: _set_cu(b, 7, _cu(b, 6) - 1))
    yield case("a negative entry", lambda b, at: _set_cu(b, 7, -5))
    yield case("last below n_tokens", lambda b, at: _set_cu(b, 65, _cu(b, 65) - 1))
    yield case("last beyond n_tokens", lambda b, at: _set_cu(b, 65, _cu(b, 65) + 1))
    yield case("a live bit at n_docs", lambda b, at: b.__setitem__(at + 8, b[at + 8] | 0x02))
    yield case("a live bit at the word's end", lambda b, at: b.__setitem__(len(b) - 1, b[-1] | 0x80))
    fields, body, _ = _body()
    yield "one byte short", fields, body[:-1]
    yield "one byte long", fields, body + b"\0"


@pytest.mark.parametrize("name,fields,body", list(_bad_bodies()), ids=[c[0] for c in _bad_bodies()])
def test_bad_bodies_are_refused_with_a_reason(name, fields, body):
    r, err = check_body(fields, body)
    assert r == -1 and err, name


def test_body_hook_checks_its_fields_first():
    fields, body, _ = _body()
    assert check_body([2] + fields[1:], body)[0] == -1 and check_body([1, 12] + fields[2:], body)[0] == -1
    L = pybert.test_lib()
    e = C.create_string_buffer(64)
    assert L.bert_hip_test_late_index_body((C.c_uint32 * 6)(*fields), bytes(body), -1, e, len(e)) == -1 and e.value
    assert L.bert_hip_test_late_index_body(None, b"", 0, e, len(e)) == -1 and e.value


def test_the_python_writer_and_parser_agree():
    rng = np.random.default_rng(3)
    cu = np.array([0, 2, 3, 7], np.int32)
    rows = rng.standard_normal((7, 16)).astype(np.float32)
    live = np.array([True, False, True])
    f = tf.parse(tf.write(rows, cu, live))
    assert (f["dim"], f["n_docs"], f["has_live"], f["n_tokens"]) == (16, 3, 1, 7)
    assert np.array_equal(f["cu"], cu) and np.array_equal(f["rows"], rows.astype(np.float16)) and f["live"].tolist() == [0b101]
    assert tf.parse(tf.write(rows, cu))["live"] is None
    r, fields, err = check(tf.write(rows, cu, live)[:64], tf.file_bytes(16, 3, 1, 7))
    assert r == 0 and check_body(fields, tf.write(rows, cu, live)[64:]) == (0, "")


# ------------------------------------------------------------------------------------------------
# the sanitizer build of the same checks, and the example's flags
# ------------------------------------------------------------------------------------------------
def test_make_check_host_passes():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bert.cpp_amd"), "check-host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("0 failure(s)") == 4 and "FAIL" not in r.stdout       # the three file programs and live_bits_cases
    assert "body: a live bit at n_docs" in r.stdout and "good, past 2^41 bytes" in r.stdout
    assert "install rejects a stray bit beyond the last row at 33" in r.stdout and "undo restores the words and the count at 1025" in r.stdout


def test_bert_search_names_the_new_flags_and_refuses_them_without_a_token_index(tmp_path):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for word in ("--save-tokens PATH", "--load-tokens PATH", "bert_hip_late_index_save", "bert_hip_late_index_load"):
        assert word in r.stderr, word
    f = tmp_path / "lines.txt"
    f.write_text("a\nb\n")
    base = [EXE, "-m", "nonexistent.bin", "-f", str(f)]
    for extra in (["--save-tokens", "x"], ["--load-tokens", "x"], ["--maxsim", "5", "--save-tokens", "x"], ["--sparse", "--load-tokens", "x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--save-tokens and --load-tokens go with --late or with --maxsim N --token-index" in r.stderr, (extra, r.stderr)
    # with a token index the flags pass the argument checks: the run fails at the model file instead (not with status 2)
    for extra in (["--late", "--save-tokens", "x"], ["--maxsim", "5", "--token-index", "--load-tokens", "x"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, 2) and "--save-tokens and" not in r.stderr, (extra, r.returncode, r.stderr)
    assert not (tmp_path / "x").exists()
