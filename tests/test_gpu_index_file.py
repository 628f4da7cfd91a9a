"""The embedding index's file form on the GPU (bert_hip_index_save / _load; the format is stated in include/bert_hip.h): a loaded
index answers with the bits of the saved one, a second save gives the same bytes, the file reads as documented with NumPy,
damaged files are refused, and bert-search --save / --load answers like the embedding run."""
import os
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = os.path.join(ROOT, "tests", "golden", "sample_client_texts_600.txt")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("removals", [False, True], ids=["whole", "with removals"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "i8"])
def test_save_load_round_trip(model, tmp_path, dtype, removals):
    rng = np.random.default_rng(41)
    N, dim, Q, k = 4500, 100, 33, 10
    rows, q = unit_rows(rng, N, dim), unit_rows(rng, Q, dim)
    allow = rng.random(N) < 0.5
    ix = model.index(dim=dim, dtype=dtype)
    ix.add(rows)
    if removals:
        gone = np.nonzero(rng.random(N) < 0.3)[0]
        ix.remove(np.concatenate([gone, np.arange(128, 1152)]))
    p1, p2 = str(tmp_path / "a.idx"), str(tmp_path / "b.idx")
    ix.save(p1)
    assert not os.path.exists(p1 + ".tmp")
    es, step = {"f32": (4, 8), "f16": (2, 16), "i8": (1, 32)}[dtype]
    dpad = (dim + step - 1) // step * step
    assert os.path.getsize(p1) == 64 + N * dpad * es + (4 * N if dtype == "i8" else 0) + (((N + 31) // 32) * 4 if removals else 0)
    ld = model.load_index(p1)
    assert (ld.dim, ld.dtype) == (dim, dtype)
    assert (len(ld), ld.n_live) == (len(ix), ix.n_live)
    assert same_bits(ld.search(q, k), ix.search(q, k))
    assert same_bits(ld.search(q, k, allow=allow), ix.search(q, k, allow=allow))
    ld.save(p2)
    with open(p1, "rb") as f1, open(p2, "rb") as f2:
        assert f1.read() == f2.read()
    # a loaded index goes on like a created one
    extra = unit_rows(rng, 40, dim)
    assert ld.add(extra) == N and ix.add(extra) == N
    assert ld.remove([N + 3, 0]) == ix.remove([N + 3, 0])
    assert same_bits(ld.search(q, k), ix.search(q, k))
    ix.close()
    ld.close()


def test_f16_file_reads_as_documented(model, tmp_path):
    rng = np.random.default_rng(43)
    N, dim = 1000, 40                                       # dpad 48, a partial last live word
    rows = unit_rows(rng, N, dim)
    ix = model.index(dim=dim, dtype="f16")
    ix.add(rows)
    gone = np.unique(rng.integers(0, N, 200))
    ix.remove(gone)
    path = str(tmp_path / "f16.idx")
    ix.save(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"BHIPIDX1"
    assert np.frombuffer(raw, "<u4", 6, 8).tolist() == [1, 1, dim, 48, N, 1]
    assert raw[32:64] == b"\0" * 32
    stored = np.frombuffer(raw, "<f2", N * 48, 64).reshape(N, 48)
    want = np.zeros((N, 48), np.float16)
    want[:, :dim] = rows.astype(np.float16)
    assert np.array_equal(stored.view(np.uint16), want.view(np.uint16))
    words = np.frombuffer(raw, "<u4", (N + 31) // 32, 64 + N * 96)
    live = np.ones(N, bool)
    live[gone] = False
    assert np.array_equal(words, pybert.allow_words(live, N))
    assert len(raw) == 64 + N * 96 + 4 * len(words)
    ix.close()


def test_i8_file_holds_codes_then_scales(model, tmp_path):
    rng = np.random.default_rng(44)
    N, dim = 70, 33                                         # dpad 64
    rows = unit_rows(rng, N, dim)
    ix = model.index(dim=dim, dtype="i8")
    ix.add(rows)
    path = str(tmp_path / "i8.idx")
    ix.save(path)
    raw = open(path, "rb").read()
    assert np.frombuffer(raw, "<u4", 6, 8).tolist() == [1, 2, dim, 64, N, 0]
    assert len(raw) == 64 + N * 64 + 4 * N
    codes = np.frombuffer(raw, np.int8, N * 64, 64).reshape(N, 64)
    scales = np.frombuffer(raw, "<f4", N, 64 + N * 64)
    amax = np.abs(rows).max(axis=1).astype(np.float32)
    assert np.array_equal(scales.view(np.int32), (amax / np.float32(127)).astype(np.float32).view(np.int32))
    assert (codes[:, dim:] == 0).all() and (np.abs(codes[:, :dim]).max(axis=1) == 127).all()
    ix.close()


def test_damaged_files_are_refused(model, tmp_path, capfd):
    rng = np.random.default_rng(45)
    ix = model.index(dim=24, dtype="f16")
    ix.add(unit_rows(rng, 100, 24))
    ix.remove([3])
    good = str(tmp_path / "good.idx")
    ix.save(good)
    ix.close()
    raw = open(good, "rb").read()
    cases = {"short": raw[:-1], "long": raw + b"\0", "magic": bytes([raw[0] ^ 0x20]) + raw[1:], "header only": raw[:64], "empty": b"",
             "live bit beyond the last row": raw[:-1] + bytes([raw[-1] | 0x80])}
    for name, data in cases.items():
        p = str(tmp_path / "bad.idx")
        with open(p, "wb") as f:
            f.write(data)
        capfd.readouterr()
        assert not model.lib.bert_hip_index_load(model.ctx, os.fsencode(p)), name
        assert "bert_hip_index_load" in capfd.readouterr().err, name
    capfd.readouterr()
    assert not model.lib.bert_hip_index_load(model.ctx, os.fsencode(str(tmp_path / "missing.idx")))
    assert "bert_hip_index_load" in capfd.readouterr().err
    ld = model.load_index(good)                             # and the good file still loads
    assert (len(ld), ld.n_live) == (100, 99)
    ld.close()


def test_search_example_save_then_load(make_model, tmp_path):
    path, _ = make_model("tiny", "f16", 0)
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")
    stdin = "Should I get health insurance?\npoaching\nq\n"
    idx = str(tmp_path / "texts.idx")

    def run(*extra, texts=TEXTS):
        return subprocess.run([exe, "-m", path, "-f", texts, *extra], input=stdin, capture_output=True, text=True, timeout=300)

    plain = run()
    saved = run("--save", idx)
    loaded = run("--load", idx)
    for r in (plain, saved, loaded):
        assert r.returncode == 0, r.stderr[-2000:]
    assert plain.stdout.count("Closest texts:") == 2 and "Loaded 600 lines." in plain.stdout
    assert saved.stdout == plain.stdout and loaded.stdout == plain.stdout
    assert os.path.getsize(idx) > 64
    # a texts file one line short of the index
    with open(TEXTS, encoding="utf-8") as f:
        lines = f.readlines()
    short = tmp_path / "short.txt"
    short.write_text("".join(lines[:-1]), encoding="utf-8")
    r = run("--load", idx, texts=str(short))
    assert r.returncode == 1 and "599" in r.stderr and "600" in r.stderr, r.stderr
