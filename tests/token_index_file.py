"""The token index's file form (include/bert_hip.h "LATE INDEX") in plain Python / NumPy, for the tests that build, damage and read
such files.  No GPU, no library."""
import struct

import numpy as np

MAGIC = b"BHIPTOK1"


def header(dim=384, n_docs=1000, has_live=1, n_tokens=25000, version=1, magic=MAGIC, reserved=b"\0" * 32):
    return magic + struct.pack("<4IQ", version, dim, n_docs, has_live, n_tokens) + reserved


def file_bytes(dim, n_docs, has_live, n_tokens):
    return 64 + (n_docs + 1) * 4 + n_tokens * dim * 2 + (-(-n_docs // 32) * 4 if has_live else 0)


def live_words(live, n_docs):
    """a bool array [n_docs] -> the uint32 words of the file (bits at and beyond n_docs zero)"""
    live = np.asarray(live, dtype=bool)
    assert live.shape == (n_docs,)
    return np.frombuffer(np.packbits(live, bitorder="little").tobytes().ljust(-(-n_docs // 32) * 4, b"\0"), dtype="<u4")


def write(rows, cu, live=None):
    """The file of documents (rows f32 [n_tokens, dim], rounded to f16 to nearest even as the index stores them; cu [n_docs + 1] from
    0) and, if live is not None, a bool array of the documents that are not removed: its bytes"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cu = np.ascontiguousarray(cu, dtype=np.int32).reshape(-1)
    n_docs, n_tokens, dim = len(cu) - 1, int(cu[-1]), rows.shape[1]
    assert cu[0] == 0 and len(rows) == n_tokens
    out = header(dim, n_docs, 0 if live is None else 1, n_tokens) + cu.astype("<i4").tobytes() + rows.astype("<f2").tobytes()
    if live is not None:
        out += live_words(live, n_docs).tobytes()
    assert len(out) == file_bytes(dim, n_docs, live is not None, n_tokens)
    return out


def parse(data):
    """A file's bytes -> dict(version, dim, n_docs, has_live, n_tokens, cu [n_docs + 1], rows f16 [n_tokens, dim], live [words] or
    None); asserts the length."""
    assert data[:8] == MAGIC
    version, dim, n_docs, has_live, n_tokens = struct.unpack("<4IQ", data[8:32])
    assert data[32:64] == b"\0" * 32 and len(data) == file_bytes(dim, n_docs, has_live, n_tokens)
    o = 64
    cu = np.frombuffer(data, "<i4", n_docs + 1, o)
    o += 4 * (n_docs + 1)
    rows = np.frombuffer(data, "<f2", n_tokens * dim, o).reshape(n_tokens, dim)
    o += 2 * n_tokens * dim
    live = np.frombuffer(data, "<u4", -(-n_docs // 32), o) if has_live else None
    return dict(version=version, dim=dim, n_docs=n_docs, has_live=has_live, n_tokens=n_tokens, cu=cu, rows=rows, live=live)
