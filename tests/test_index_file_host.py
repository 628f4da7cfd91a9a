"""The embedding index's file form and its new entry points without a GPU: the header check bert_hip_index_load runs before it
allocates (bert_hip_test_index_header; the format is stated in include/bert_hip.h), what the entry points answer without an
index, and bert-search's options."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ELEM = {0: 4, 1: 2, 2: 1}
STEP = {0: 8, 1: 16, 2: 32}


def dpad_of(dtype, dim):
    return (dim + STEP[dtype] - 1) // STEP[dtype] * STEP[dtype]


def header(dtype=1, dim=384, n_rows=1000, has_live=0, version=1, dpad=None, magic=b"BHIPIDX1", reserved=b"\0" * 32):
    dpad = dpad_of(dtype, dim) if dpad is None and dtype in STEP else (dpad or 0)
    return magic + struct.pack("<6I", version, dtype, dim, dpad, n_rows, has_live) + reserved


def file_bytes(dtype, dim, n_rows, has_live):
    n = 64 + n_rows * dpad_of(dtype, dim) * ELEM[dtype]
    if dtype == 2:
        n += 4 * n_rows
    if has_live:
        n += (n_rows + 31) // 32 * 4
    return n


def check(buf, size):
    fields = (C.c_uint32 * 6)(*([0xFFFFFFFF] * 6))
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_index_header(buf, len(buf), size, fields, err, len(err))
    return r, list(fields), err.value.decode()


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("dim,n_rows,has_live", [(384, 1000, 0), (7, 33, 1), (2048, 0, 0), (1, 1, 1)])
def test_good_headers_are_accepted(dtype, dim, n_rows, has_live):
    r, fields, err = check(header(dtype, dim, n_rows, has_live), file_bytes(dtype, dim, n_rows, has_live))
    assert r == 0 and err == "", err
    assert fields == [1, dtype, dim, dpad_of(dtype, dim), n_rows, has_live]


def _bad_cases():
    good = file_bytes(1, 384, 1000, 0)
    yield "short buffer", header()[:63], good
    yield "wrong magic", header(magic=b"BHIPIDX2"), good
    yield "flipped magic bit", bytes([header()[0] ^ 1]) + header()[1:], good
    yield "version 2", header(version=2), good
    yield "dtype 3", header(dtype=3, dpad=384), good
    yield "dim 0", header(dim=0), 64
    yield "dim 2049", header(dim=2049, n_rows=0), 64
    yield "dpad not create's (f16, 384 -> 400)", header(dpad=400), 64 + 1000 * 400 * 2
    yield "dpad not create's (i8 stored with the f16 step)", header(dtype=2, dim=40, dpad=48, n_rows=10), 64 + 10 * 48 + 40
    yield "non-zero reserved byte", header(reserved=b"\0" * 31 + b"\1"), good
    yield "non-zero first reserved byte", header(reserved=b"\1" + b"\0" * 31), good
    yield "file one byte short", header(), good - 1
    yield "file one byte long", header(), good + 1
    yield "i8 file without its scales", header(dtype=2), file_bytes(2, 384, 1000, 0) - 4000
    yield "has_live = 1 without the bitmap", header(has_live=1), good
    yield "has_live = 2", header(has_live=2), file_bytes(1, 384, 1000, 1)


@pytest.mark.parametrize("name,buf,size", list(_bad_cases()), ids=[c[0] for c in _bad_cases()])
def test_bad_headers_are_rejected_with_a_message(name, buf, size):
    r, fields, err = check(buf, size)
    assert r == -1, name
    assert err, name
    assert fields == [0xFFFFFFFF] * 6                      # nothing written on a refusal


def test_entry_points_without_an_index_or_a_device(sparse_vocab_model, tmp_path, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        path = tmp_path / "x.idx"
        path.write_bytes(header(1, 8, 0, 0))               # a valid, empty f16 index
        capfd.readouterr()
        assert not m.lib.bert_hip_index_load(m.ctx, os.fsencode(str(path)))
        assert "bert_hip_index_load" in capfd.readouterr().err
        with pytest.raises(RuntimeError, match="bert_hip_index_load"):
            m.load_index(str(path))
        L = m.lib
        ids = np.zeros(4, np.int32)
        sc = np.zeros(4, np.float32)
        q = np.zeros(8, np.float32)
        words = np.ones(1, np.uint32)
        assert L.bert_hip_index_remove(None, 1, ids.ctypes.data_as(C.POINTER(C.c_int32))) < 0
        assert L.bert_hip_index_n_live(None) == -1
        assert L.bert_hip_index_save(None, os.fsencode(str(tmp_path / "y.idx"))) < 0
        assert not (tmp_path / "y.idx").exists()
        assert L.bert_hip_index_compact(None, None) < 0
        assert L.bert_hip_index_search_filtered(None, 1, q.ctypes.data_as(C.POINTER(C.c_float)), 4, words.ctypes.data, 1,
                                                ids.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_float))) < 0
        assert L.bert_hip_index_search_filtered_device(None, 1, None, 4, None, 0, None, None, None) < 0
        assert (ids == 0).all() and (sc == 0).all()
    finally:
        m.close()


def test_allow_words_packing():
    a = np.zeros(70, bool)
    a[[0, 31, 32, 69]] = True
    assert pybert.allow_words(a, 70).tolist() == [0x80000001, 0x1, 0x20]
    w = np.array([5, 6, 7], np.uint32)
    assert pybert.allow_words(w, 70) is not None and pybert.allow_words(w, 70).tolist() == [5, 6, 7]      # words pass through
    with pytest.raises(ValueError):
        pybert.allow_words(np.zeros(69, bool), 70)


def test_search_example_usage_names_save_and_load():
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    usage = [line for line in r.stderr.splitlines() if line.startswith("usage:")]
    assert usage and all(opt in usage[0] for opt in ("--save", "--load", "--i8")), r.stderr
