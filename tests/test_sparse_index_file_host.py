"""The sparse index's file form and its new entry points without a GPU: the header and body checks bert_hip_sparse_index_load runs
(sparse_index_file.h through bert_hip_test_sparse_index_header / _body; the format is stated in include/bert_hip.h), the new symbols,
and what every new entry point answers without an index or on a tokenizer-only context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bert_cpp_amd import pybert

import sparse_index_file as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bert_hip_sparse_index_remove", "bert_hip_sparse_index_n_live", "bert_hip_sparse_index_search_filtered",
               "bert_hip_sparse_index_search_filtered_device", "bert_hip_sparse_index_rescore", "bert_hip_sparse_index_rescore_device",
               "bert_hip_sparse_index_compact", "bert_hip_sparse_index_save", "bert_hip_sparse_index_load"]
HOOKS = ["bert_hip_test_sparse_index_header", "bert_hip_test_sparse_index_body"]


def check(buf, size):
    fields = (C.c_uint32 * 6)(*([0xFFFFFFFF] * 6))
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_sparse_index_header(buf, len(buf), size, fields, err, len(err))
    return r, list(fields), err.value.decode()


def check_body(fields, body):
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_sparse_index_body((C.c_uint32 * 6)(*fields), bytes(body), len(body), err, len(err))
    return r, err.value.decode()


# ------------------------------------------------------------------------------------------------
# the header
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n_vocab,width,n_rows,has_live", [
    (0, 30522, 128, 1000, 1), (1, 30522, 128, 1000, 0), (0, 1, 1, 0, 0), (0, 1, 1, 0, 1), (1, 65536, 256, 65, 1), (0, 262144, 4, 300, 0),
    # byte counts beyond 32 bits: 2^24 rows of 128 i32 + f32 terms are 2^34 bytes of blocks; the largest file needs 41 bits
    (0, 30522, 128, 2 ** 24, 1), (1, 65536, 256, 2 ** 31 - 65, 1), (0, 262144, 256, 2 ** 31 - 65, 1)])
def test_good_headers_are_accepted(dtype, n_vocab, width, n_rows, has_live):
    assert len(sf.header()) == 64
    size = sf.file_bytes(dtype, width, n_rows, has_live)
    r, fields, err = check(sf.header(dtype, n_vocab, width, n_rows, has_live), size)
    assert r == 0 and err == "", err
    assert fields == [1, dtype, n_vocab, width, n_rows, has_live]


def test_file_length_arithmetic():
    assert sf.file_bytes(0, 128, 1000, 1) == 64 + 2 * 16 * 128 * 64 * 4 + 4000 + 32 * 4
    assert sf.file_bytes(1, 7, 65, 0) == 64 + 2 * 2 * 7 * 64 * 2 + 260
    assert sf.file_bytes(0, 1, 0, 1) == 64
    big = sf.file_bytes(0, 256, 2 ** 31 - 65, 1)
    assert big == 64 + 2 * (2 ** 25 - 1) * 256 * 64 * 4 + (2 ** 31 - 65) * 4 + 2 ** 26 * 4 - 8 and big > 2 ** 41


def _bad_cases():
    good = sf.file_bytes(0, 128, 1000, 1)
    yield "wrong magic", sf.header(magic=b"BHIPIDX1"), good
    yield "flipped magic bit", bytes([sf.header()[0] ^ 1]) + sf.header()[1:], good
    yield "version 2", sf.header(version=2), good
    yield "dtype 2", sf.header(dtype=2), good
    yield "width 0", sf.header(width=0), sf.file_bytes(0, 0, 1000, 1)
    yield "width 257", sf.header(width=257), sf.file_bytes(0, 257, 1000, 1)
    yield "n_vocab 0", sf.header(n_vocab=0), good
    yield "n_vocab 262145", sf.header(n_vocab=262145), good
    yield "dtype 1 with n_vocab 65537", sf.header(dtype=1, n_vocab=65537), sf.file_bytes(1, 128, 1000, 1)
    yield "a reserved byte set (last)", sf.header(reserved=b"\0" * 31 + b"\1"), good
    yield "a reserved byte set (first)", sf.header(reserved=b"\1" + b"\0" * 31), good
    yield "has_live 2", sf.header(has_live=2), good
    yield "n_rows 2^31 - 64", sf.header(n_rows=2 ** 31 - 64), sf.file_bytes(0, 128, 2 ** 31 - 64, 1)
    yield "short buffer", sf.header()[:63], good
    yield "one byte", sf.header()[:1], 1
    yield "empty buffer", b"", good
    yield "truncated by one byte", sf.header(), good - 1
    yield "one byte long", sf.header(), good + 1
    yield "header only", sf.header(), 64
    yield "has_live set, the words missing", sf.header(), sf.file_bytes(0, 128, 1000, 0)
    big = sf.file_bytes(0, 256, 2 ** 31 - 65, 1)
    yield "a length that equals the header's modulo 2^32", sf.header(0, 262144, 256, 2 ** 31 - 65, 1), big % 2 ** 32
    # 2^24 rows: the two block arrays are exactly 2^34 bytes, 0 modulo 2^32
    yield "blocks whose bytes wrap to 0 modulo 2^32", sf.header(n_rows=2 ** 24), sf.file_bytes(0, 128, 2 ** 24, 1) - 2 ** 34


@pytest.mark.parametrize("name,buf,size", list(_bad_cases()), ids=[c[0] for c in _bad_cases()])
def test_bad_headers_are_rejected_with_a_reason(name, buf, size):
    r, fields, err = check(buf, size)
    assert r == -1, name
    assert err, name
    assert fields == [0xFFFFFFFF] * 6                      # nothing written on a refusal


def test_negative_lengths_are_refused():
    L = pybert.test_lib()
    err = C.create_string_buffer(64)
    assert L.bert_hip_test_sparse_index_header(sf.header(), -1, 64, None, err, len(err)) == -1 and err.value
    assert L.bert_hip_test_sparse_index_header(sf.header(), 64, -1, None, err, len(err)) == -1 and err.value
    assert L.bert_hip_test_sparse_index_body((C.c_uint32 * 6)(1, 0, 64, 4, 0, 0), b"", -1, err, len(err)) == -1 and err.value
    assert L.bert_hip_test_sparse_index_body(None, b"", 0, err, len(err)) == -1 and err.value


# ------------------------------------------------------------------------------------------------
# the body
# ------------------------------------------------------------------------------------------------
def make_body(dtype, n_vocab, width, n_rows, has_live):
    """(fields, body bytearray, set_count, set_id): row r holds r % (width + 1) terms with ids 0, 1, ..., every row live"""
    eb = 2 if dtype == 1 else 4
    arr = sf.array_bytes(dtype, width, n_rows)
    body = bytearray(sf.file_bytes(dtype, width, n_rows, has_live) - 64)

    def set_count(r, n):
        body[2 * arr + 4 * r:2 * arr + 4 * r + 4] = int(n & 0xFFFFFFFF).to_bytes(4, "little")

    def set_id(r, j, v):
        o = ((r // 64 * width + j) * 64 + r % 64) * eb
        body[o:o + eb] = int(v & (2 ** (8 * eb) - 1)).to_bytes(eb, "little")

    for r in range(n_rows):
        set_count(r, r % (width + 1))
        for j in range(r % (width + 1)):
            set_id(r, j, j % n_vocab)
        if has_live:
            body[2 * arr + 4 * n_rows + r // 8] |= 1 << (r % 8)
    return [1, dtype, n_vocab, width, n_rows, has_live], body, set_count, set_id


@pytest.mark.parametrize("dtype", [0, 1])
def test_body_checks(dtype):
    for n_rows, width, has_live in ((0, 4, 0), (1, 4, 1), (65, 4, 1), (300, 256, 1), (64, 4, 1)):
        fields, body, _, _ = make_body(dtype, 300, width, n_rows, has_live)
        assert check_body(fields, body) == (0, ""), (n_rows, width)
    fields, body, set_count, set_id = make_body(dtype, 64, 4, 65, 1)
    assert check_body(fields, body[:-1])[0] == -1 and check_body(fields, body + b"\0")[0] == -1

    def bad(change, what):
        fields, body, set_count, set_id = make_body(dtype, 64, 4, 65, 1)
        change(body, set_count, set_id)
        r, err = check_body(fields, body)
        assert r == -1 and what in err, (what, err)

    bad(lambda b, c, i: c(64, 5), "count 5")
    bad(lambda b, c, i: c(3, -1), "count -1")
    bad(lambda b, c, i: i(64, 3, 64), "id 64")                            # row 64 holds 4 terms: column 3 is used
    bad(lambda b, c, i: i(4, 0, 64), "id 64")
    bad(lambda b, c, i: b.__setitem__(len(b) - 1, b[-1] | 0x80), "live bits")
    if dtype == 0:
        bad(lambda b, c, i: i(64, 3, -1), "id -1")
    # what is not looked at: an id behind its row's count, a row of the last block beyond n_rows, the weights
    fields, body, set_count, set_id = make_body(dtype, 64, 4, 65, 1)
    set_id(5, 3, 0xFFFF)                                                  # row 5 holds no term
    set_id(66, 0, 0xFFFF)
    arr = sf.array_bytes(dtype, 4, 65)
    body[arr:2 * arr] = b"\xff" * arr                                     # NaN weights load as they are
    assert check_body(fields, body) == (0, "")
    # n_vocab - 1 is a legal id; a removed last row of a full word is legal
    fields, body, set_count, set_id = make_body(dtype, 64, 4, 64, 1)
    set_id(63, 2, 63)
    body[-1] &= 0x7F
    assert check_body(fields, body) == (0, "")
    # the fields pass the header check first
    assert check_body([1, dtype, 64, 257, 0, 0], b"")[0] == -1 and check_body([2, dtype, 64, 4, 0, 0], b"")[0] == -1


# ------------------------------------------------------------------------------------------------
# symbols
# ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    L, T = pybert.lib(), pybert.test_lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pybert.BERT_HIP_H_SYMBOLS, sym
        assert hasattr(L, sym) and hasattr(T, sym), sym
    test_text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    for hook in HOOKS:
        assert hook in test_text and hook in pybert.BERT_HIP_TEST_H_SYMBOLS
        assert hasattr(T, hook) and not hasattr(L, hook)
    assert "BHIPSPX1" in text


def test_binding_has_the_new_methods_with_todays_defaults():
    import inspect
    sig = inspect.signature(pybert.BertSparseIndex.search)
    assert sig.parameters["allow"].default is None and list(sig.parameters)[:4] == ["self", "q_ids", "q_weights", "k"]
    sig = inspect.signature(pybert.BertSparseIndex.search_device)
    assert sig.parameters["d_allow_ptr"].default == 0 and sig.parameters["n_words"].default == 0
    assert list(sig.parameters)[:9] == ["self", "n_queries", "kq", "d_q_ids_ptr", "d_q_weights_ptr", "k", "d_ids_ptr", "d_scores_ptr", "stream"]
    for name in ("remove", "compact", "save", "rescore", "rescore_device", "live_ids"):
        assert callable(getattr(pybert.BertSparseIndex, name))
    assert isinstance(pybert.BertSparseIndex.n_live, property) and callable(pybert.BertModel.load_sparse_index)


# ------------------------------------------------------------------------------------------------
# refusals that need no device
# ------------------------------------------------------------------------------------------------
def test_null_index_and_null_context(tmp_path, capfd):
    L = pybert.lib()
    ids = np.full((1, 4), 7, np.int32)
    w = np.full((1, 4), 7.0, np.float32)
    words = np.ones(1, np.uint32)
    p = lambda a: a.ctypes.data
    path = os.fsencode(str(tmp_path / "x.spx"))
    capfd.readouterr()
    assert L.bert_hip_sparse_index_n_live(None) == -1                    # (like size: no line)
    assert capfd.readouterr().err == ""
    assert L.bert_hip_sparse_index_remove(None, 1, p(ids)) == -1
    assert L.bert_hip_sparse_index_search_filtered(None, 1, 4, p(ids), p(w), 4, p(words), 1, p(ids), p(w)) == -1
    assert L.bert_hip_sparse_index_search_filtered_device(None, 1, 4, None, None, 4, None, 0, None, None, None) == -1
    assert L.bert_hip_sparse_index_rescore(None, 1, 4, p(ids), p(w), 4, p(ids), 4, p(ids), p(w)) == -1
    assert L.bert_hip_sparse_index_rescore_device(None, 1, 4, None, None, 4, None, 4, None, None, None) == -1
    assert L.bert_hip_sparse_index_compact(None, p(ids)) == -1
    assert L.bert_hip_sparse_index_save(None, path) == -1
    err = capfd.readouterr().err
    for name in ("remove", "search_filtered", "search_filtered_device", "rescore", "rescore_device", "compact", "save"):
        assert f"bert_hip_sparse_index_{name}: no index" in err, name
    assert len(err.strip().splitlines()) == 7                            # one line each, nothing else
    assert not L.bert_hip_sparse_index_load(None, path)
    assert "no context" in capfd.readouterr().err
    assert (ids == 7).all() and (w == 7.0).all()
    assert not (tmp_path / "x.spx").exists() and not (tmp_path / "x.spx.tmp").exists()


def test_tokenizer_only_context_loads_no_sparse_index(sparse_vocab_model, tmp_path, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        good = tmp_path / "empty.spx"
        good.write_bytes(sf.header(0, 64, 4, 0, 0))                       # a valid file of an empty index
        capfd.readouterr()
        assert not m.lib.bert_hip_sparse_index_load(m.ctx, os.fsencode(str(good)))
        assert "tokenizer-only" in capfd.readouterr().err
        with pytest.raises(RuntimeError):
            m.load_sparse_index(str(good))
    finally:
        m.close()
