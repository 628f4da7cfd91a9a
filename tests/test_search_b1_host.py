"""The 1-bit index form (dtype 3, "b1") and the rescoring entry points without a GPU: the file header check at dtype 3 (a row
is dpad / 8 bytes, dpad = dim rounded up to 128, no scale block), bert-search's options, the binding's dtype name, and what
the new entry points answer without an index."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dpad_of(dim, step=128):
    return (dim + step - 1) // step * step


def header(dim, n_rows, has_live, dpad=None):
    return b"BHIPIDX1" + struct.pack("<6I", 1, 3, dim, dpad_of(dim) if dpad is None else dpad, n_rows, has_live) + b"\0" * 32


def file_bytes(dim, n_rows, has_live, dpad=None):
    n = 64 + n_rows * (dpad_of(dim) if dpad is None else dpad) // 8
    return n + ((n_rows + 31) // 32 * 4 if has_live else 0)


def check(buf, size):
    fields = (C.c_uint32 * 6)(*([0xFFFFFFFF] * 6))
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_index_header(buf, len(buf), size, fields, err, len(err))
    return r, list(fields), err.value.decode()


CASES = [(384, 1000, 0), (7, 33, 1), (2048, 0, 0), (1, 1, 1)]


@pytest.mark.parametrize("dim,n_rows,has_live", CASES)
def test_b1_headers_are_accepted_at_the_stated_length(dim, n_rows, has_live):
    r, fields, err = check(header(dim, n_rows, has_live), file_bytes(dim, n_rows, has_live))
    assert r == 0 and err == "", err
    assert fields == [1, 3, dim, dpad_of(dim), n_rows, has_live]


def test_b1_file_length_at_dim_384_is_48_bytes_per_row():
    assert file_bytes(384, 1000, 0) == 64 + 1000 * 48


@pytest.mark.parametrize("dim,n_rows,has_live", CASES)
@pytest.mark.parametrize("off", [-1, 1])
def test_b1_files_one_byte_short_or_long_are_refused(dim, n_rows, has_live, off):
    r, fields, err = check(header(dim, n_rows, has_live), file_bytes(dim, n_rows, has_live) + off)
    assert r == -1 and err
    assert ("truncated" if off < 0 else "over-long") in err
    assert fields == [0xFFFFFFFF] * 6


@pytest.mark.parametrize("dim,n_rows,has_live", [c for c in CASES if dpad_of(c[0], 32) != dpad_of(c[0])])
def test_b1_dpad_rounded_to_32_is_refused(dim, n_rows, has_live):
    dpad = dpad_of(dim, 32)
    r, fields, err = check(header(dim, n_rows, has_live, dpad=dpad), file_bytes(dim, n_rows, has_live, dpad=dpad))
    assert r == -1 and "dpad" in err
    assert fields == [0xFFFFFFFF] * 6


def test_b1_file_with_a_scale_block_is_refused():
    r, _, err = check(header(384, 1000, 0), file_bytes(384, 1000, 0) + 4000)
    assert r == -1 and "over-long" in err


def test_dtype_4_is_refused():
    buf = b"BHIPIDX1" + struct.pack("<6I", 1, 4, 384, 384, 0, 0) + b"\0" * 32
    r, _, err = check(buf, 64)
    assert r == -1 and "dtype 4" in err


def test_search_example_usage_names_b1_and_rescore():
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    usage = [line for line in r.stderr.splitlines() if line.startswith("usage:")]
    assert usage and all(opt in usage[0] for opt in ("--b1", "--rescore", "--i8", "--save", "--load")), r.stderr


def test_b1_is_a_dtype_of_the_binding(sparse_vocab_model, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        capfd.readouterr()
        # the name is accepted and the call reaches bert_hip_index_create, which refuses a context without a device
        with pytest.raises(RuntimeError, match="bert_hip_index_create"):
            m.index(dtype="b1")
        assert "bert_hip_index_create" in capfd.readouterr().err
        with pytest.raises(ValueError, match="'i8'.*'b1'"):
            m.index(dtype="b2")
    finally:
        m.close()


def test_new_entry_points_without_an_index_leave_the_outputs():
    L = pybert.lib()
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ids = np.full(4, 7, np.int32)
    sc = np.full(4, 0.5, np.float32)
    q = np.zeros(8, np.float32)
    cand = np.zeros(2, np.int32)
    outs = (ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
    assert L.bert_hip_index_rescore(None, 1, q.ctypes.data_as(f32p), 2, cand.ctypes.data_as(i32p), 4, *outs) < 0
    assert L.bert_hip_index_rescore_device(None, 1, None, 2, None, 4, None, None, None) < 0
    assert L.bert_hip_index_search_rescored(None, None, 1, q.ctypes.data_as(f32p), 4, 4, *outs) < 0
    assert L.bert_hip_index_search_rescored_device(None, None, 1, None, 4, 4, None, None, None) < 0
    assert (ids == 7).all() and (sc == 0.5).all()
