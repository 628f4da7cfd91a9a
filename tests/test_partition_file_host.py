"""The partition file and the new probed entry points without a GPU: the header check bert_hip_index_partition_load runs before it
reads or allocates (index_file.h partition_header_check through bert_hip_test_partition_header; the format is stated in
include/bert_hip.h), what the six new entry points answer without an index, and bert-search's usage text."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(dim=384, n_lists=1024, n_part=100000, version=1, magic=b"BHIPPRT1", reserved=b"\0" * 40):
    return magic + struct.pack("<4I", version, dim, n_lists, n_part) + reserved


def file_bytes(dim, n_lists, n_part):
    return 64 + n_lists * dim * 4 + n_part * 4


def check(buf, size):
    fields = (C.c_uint32 * 4)(*([0xFFFFFFFF] * 4))
    err = C.create_string_buffer(256)
    r = pybert.test_lib().bert_hip_test_partition_header(buf, len(buf), size, fields, err, len(err))
    return r, list(fields), err.value.decode()


@pytest.mark.parametrize("dim,n_lists,n_part", [(384, 1024, 100000), (1, 1, 0), (2048, 65536, 7), (72, 12, 1500),
                                                 (384, 1024, 2 ** 31 - 1), (2048, 65536, 2 ** 31 - 1)])
def test_good_headers_are_accepted(dim, n_lists, n_part):
    assert len(header()) == 64
    r, fields, err = check(header(dim, n_lists, n_part), file_bytes(dim, n_lists, n_part))
    assert r == 0 and err == "", err
    assert fields == [1, dim, n_lists, n_part]


def _bad_cases():
    good = file_bytes(384, 1024, 100000)
    yield "wrong magic", header(magic=b"BHIPIDX1"), good
    yield "flipped magic bit", bytes([header()[0] ^ 1]) + header()[1:], good
    yield "version 2", header(version=2), good
    yield "dim 0", header(dim=0), file_bytes(0, 1024, 100000)
    yield "dim 2049", header(dim=2049), file_bytes(2049, 1024, 100000)
    yield "n_lists 0", header(n_lists=0), file_bytes(384, 0, 100000)
    yield "n_lists 65537", header(n_lists=65537), file_bytes(384, 65537, 100000)
    yield "n_part 2^31", header(n_part=2 ** 31), file_bytes(384, 1024, 2 ** 31)
    yield "non-zero last reserved byte", header(reserved=b"\0" * 39 + b"\1"), good
    yield "non-zero first reserved byte", header(reserved=b"\1" + b"\0" * 39), good
    yield "short buffer", header()[:63], good
    yield "empty buffer", b"", good
    yield "file one byte short", header(), good - 1
    yield "file one byte long", header(), good + 1
    yield "header only", header(), 64
    # 64 + 65536 * 2048 * 4 + (2^31 - 1) * 4 needs 34 bits: the length taken modulo 2^32 is another, much shorter file
    big = file_bytes(2048, 65536, 2 ** 31 - 1)
    assert big >= 2 ** 33
    yield "a length that equals the header's modulo 2^32", header(2048, 65536, 2 ** 31 - 1), big % 2 ** 32
    yield "n_part whose bytes alone wrap to 0 modulo 2^32", header(384, 1024, 2 ** 30), file_bytes(384, 1024, 0)


@pytest.mark.parametrize("name,buf,size", list(_bad_cases()), ids=[c[0] for c in _bad_cases()])
def test_bad_headers_are_rejected_with_a_reason(name, buf, size):
    r, fields, err = check(buf, size)
    assert r == -1, name
    assert err, name
    assert fields == [0xFFFFFFFF] * 4                      # nothing written on a refusal


def test_negative_lengths_are_refused():
    L = pybert.test_lib()
    err = C.create_string_buffer(64)
    assert L.bert_hip_test_partition_header(header(), -1, 64, None, err, len(err)) == -1 and err.value
    assert L.bert_hip_test_partition_header(header(), 64, -1, None, err, len(err)) == -1 and err.value


def test_new_entry_points_refuse_a_missing_index(sparse_vocab_model, tmp_path, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        L = m.lib
        ids = np.zeros(4, np.int32)
        f = np.full(8, 0.5, np.float32)
        words = np.ones(1, np.uint32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        pi, pf = ids.ctypes.data_as(i32p), f.ctypes.data_as(f32p)
        path = os.fsencode(str(tmp_path / "x.part"))
        capfd.readouterr()
        assert L.bert_hip_index_search_probed_filtered(None, 1, pf, 1, 1, words.ctypes.data, 1, pi, pf) == -1
        assert L.bert_hip_index_search_probed_filtered_device(None, 1, None, 1, 1, None, 0, None, None, None) == -1
        assert L.bert_hip_index_search_rescored_probed(None, None, 1, pf, 1, 1, 1, words.ctypes.data, 1, pi, pf) == -1
        assert L.bert_hip_index_search_rescored_probed_device(None, None, 1, None, 1, 1, 1, None, 0, None, None, None) == -1
        assert L.bert_hip_index_partition_save(None, path) == -1
        assert L.bert_hip_index_partition_load(None, path) == -1
        err = capfd.readouterr().err
        for name in ("search_probed_filtered", "search_probed_filtered_device", "search_rescored_probed", "search_rescored_probed_device",
                     "partition_save", "partition_load"):
            assert f"bert_hip_index_{name}: no index" in err, name
        assert len(err.strip().splitlines()) == 6                        # one line each, nothing else
        assert (ids == 0).all() and (f == 0.5).all()
        assert not (tmp_path / "x.part").exists() and not (tmp_path / "x.part.tmp").exists()
    finally:
        m.close()


def test_binding_has_the_new_methods_with_todays_defaults():
    import inspect
    sig = inspect.signature(pybert.BertIndex.search_probed)
    assert sig.parameters["allow"].default is None and list(sig.parameters)[:4] == ["self", "queries", "k", "nprobe"]
    sig = inspect.signature(pybert.BertIndex.search_probed_device)
    assert sig.parameters["d_allow_ptr"].default == 0 and sig.parameters["n_words"].default == 0
    for name in ("search_rescored_probed", "search_rescored_probed_device", "save_partition", "load_partition"):
        assert callable(getattr(pybert.BertIndex, name))


def test_search_example_usage_names_the_probed_rescore():
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    usage = [line for line in r.stderr.splitlines() if line.startswith("usage:")]
    assert usage and all(opt in usage[0] for opt in ("--rescore", "--lists", "--nprobe", "--save", "--load")), r.stderr
    # --nprobe together with --rescore is no longer refused at the command line: the run gets as far as the model file
    r = subprocess.run([exe, "-m", "/nonexistent/model.bin", "-f", "/nonexistent/texts", "--b1", "--rescore", "10", "--lists", "4", "--nprobe", "2"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "goes without --rescore" not in r.stderr and "failed to load model" in r.stderr, r.stderr
