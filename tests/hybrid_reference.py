"""The hybrid search's contract in plain NumPy (include/bert_hip.h "Hybrid search"): the score rule and the reference of a result.  No
GPU, no library.

H = (w_dense * D) + (w_sparse * S): two float32 multiplications and one float32 addition, each rounded once to nearest even — NumPy's
float32 arithmetic —, never an fma.  D and S are the two indexes' own score bits; the top-k is sparse_index_reference.topk (larger
score first, equal scores by smaller id, NaN never returned, id -1 / score -inf beyond)."""
import numpy as np

import sparse_index_reference as sref


def combine(D, S, wd, ws):
    """H over arrays of one shape, float32 throughout"""
    D, S = np.asarray(D, np.float32), np.asarray(S, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.float32(wd) * D
        y = np.float32(ws) * S
        return (x + y).astype(np.float32)


def search(D, S, qual, wd, ws, k):
    """(ids [nq][k], scores [nq][k]): D, S [nq][n] the dense and the sparse score bits, qual [n] bool the rows that qualify (the
    others' scores become NaN, which topk never returns)"""
    H = combine(D, S, wd, ws)
    H[:, ~np.asarray(qual, bool)] = np.nan
    res = [sref.topk(row, k) for row in H]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def chunk_queries(n_rows, nq, pref=0):
    """(HC, ld) as sparse_index_kernels.h hybrid_chunk_queries states them: ld = n_rows rounded up to 64 floats; HC the most queries
    whose [HC][ld] f32 matrix fits 256 MiB, at most nq and 4096, at least 1, a multiple of 32 from 32 on; pref > 0: that chunk size
    instead, unrounded, under the same bounds"""
    ld = (n_rows + 63) // 64 * 64
    hc = min((256 << 20) // (max(ld, 64) * 4), nq, 4096)
    if pref > 0:
        hc = min(hc, pref)
    elif hc >= 32:
        hc = hc // 32 * 32
    return max(hc, 1), ld
