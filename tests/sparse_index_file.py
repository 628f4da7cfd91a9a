"""The sparse index's file form (include/bert_hip.h "Sparse index: removing rows ... files") in plain Python / NumPy, for the tests
that build, damage and read such files.  No GPU, no library."""
import struct

import numpy as np

MAGIC = b"BHIPSPX1"


def header(dtype=0, n_vocab=30522, width=128, n_rows=1000, has_live=1, version=1, magic=MAGIC, reserved=b"\0" * 32):
    return magic + struct.pack("<6I", version, dtype, n_vocab, width, n_rows, has_live) + reserved


def array_bytes(dtype, width, n_rows):
    """bytes of the id blocks, and of the weight blocks: ceil(n_rows / 64) blocks of [width][64] elements"""
    return -(-n_rows // 64) * width * 64 * (2 if dtype == 1 else 4)


def file_bytes(dtype, width, n_rows, has_live):
    return 64 + 2 * array_bytes(dtype, width, n_rows) + n_rows * 4 + (-(-n_rows // 32) * 4 if has_live else 0)


def parse(data):
    """A file's bytes -> dict(fields..., ids [blocks][width][64], weights the same, counts [n_rows], live [words] or None); asserts
    the length."""
    assert data[:8] == MAGIC
    version, dtype, n_vocab, width, n_rows, has_live = struct.unpack("<6I", data[8:32])
    assert data[32:64] == b"\0" * 32 and len(data) == file_bytes(dtype, width, n_rows, has_live)
    arr = array_bytes(dtype, width, n_rows)
    blocks = -(-n_rows // 64)
    it, wt = ("<u2", "<f2") if dtype == 1 else ("<i4", "<f4")
    o = 64
    ids = np.frombuffer(data, it, blocks * width * 64, o).reshape(blocks, width, 64)
    o += arr
    weights = np.frombuffer(data, wt, blocks * width * 64, o).reshape(blocks, width, 64)
    o += arr
    counts = np.frombuffer(data, "<i4", n_rows, o)
    o += 4 * n_rows
    live = np.frombuffer(data, "<u4", -(-n_rows // 32), o) if has_live else None
    return dict(version=version, dtype=dtype, n_vocab=n_vocab, width=width, n_rows=n_rows, has_live=has_live, ids=ids, weights=weights,
                counts=counts, live=live)


def rows_of(f):
    """the rows of a parsed file as get_rows returns them: (ids [n][width] ascending then -1, weights [n][width] f32, +0 behind)"""
    n, width = f["n_rows"], f["width"]
    ids = f["ids"].transpose(0, 2, 1).reshape(-1, width)[:n].astype(np.int32)
    w = f["weights"].transpose(0, 2, 1).reshape(-1, width)[:n].astype(np.float32)
    used = np.arange(width)[None, :] < f["counts"][:, None]
    return np.where(used, ids, -1).astype(np.int32), np.where(used, w, np.float32(0)).astype(np.float32)
