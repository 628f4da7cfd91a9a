"""References and case builders for the token index (include/bert_hip.h "TOKEN INDEX"; tests: test_token_index_host.py,
test_gpu_token_index.py).  No GPU.

Scores.  The float64 score of a (query, document) pair and its bound are maxsim_reference.pair_reference's, on the f16-rounded rows.
Results.  What a search or a rescore must return is the indexes' order rule (index_reference.ref_topk through topk_order_reference)
applied to a GIVEN score matrix — in the GPU tests the matrix bert_hip_maxsim gives for all pairs of the same rows, so ids must be
equal and scores equal in bits wherever they are not zero.
The plan.  plan() restates token_index_kernels.h token_index_plan in Python; the host test holds the hook against it."""
import numpy as np

import maxsim_reference as mr
import topk_order_reference as tor

TARGET_BLOCKS = 2048
MIN_SLICE_DOCS = 16
MAX_SLICES = 4096
DOC_LENS = [1, 2, 31, 32, 33, 64, 65, 96, 130, 513]       # the lengths the GPU tests' documents cycle through
QUERY_LENS = [1, 31, 32, 33, 64, 96, 128]


def max_query_tokens(dim):
    """the largest multiple of 32, at most 128, whose blocks of 32 (dim + 8) halfs fit 160 KiB - 256 bytes beside a list of 512 entries"""
    return min(128, (160 * 1024 - 256 - 512 * 8 - 16) // (64 * (dim + 8)) * 32)


def plan(n_docs, nq, pref=0):
    """(n_slices, slice_docs), or None where the plan refuses"""
    if n_docs < 0 or nq < 1 or not 0 <= pref <= MAX_SLICES:
        return None
    aim = min(pref, max(n_docs, 1)) if pref > 0 else max(1, min((TARGET_BLOCKS + nq - 1) // nq, n_docs // MIN_SLICE_DOCS))
    slice_docs = max(1, (n_docs + aim - 1) // aim)
    return max(1, (n_docs + slice_docs - 1) // slice_docs), slice_docs


def slices_of(n_docs, n_slices, slice_docs):
    """the document ranges [r0, r1) the kernel gives its slices"""
    out = []
    for s in range(n_slices):
        r0 = min(s * slice_docs, n_docs)
        out.append((r0, min(r0 + slice_docs, n_docs)))
    return out


def scores_f64(q, qcu, d, dcu):
    """(scores, bounds) float64 [n_q, n_d] of the f16-rounded rows (maxsim_reference.pair_reference per pair)"""
    return mr.maxsim_reference(mr.round_f16(q), qcu, mr.round_f16(d), dcu)


def search_expected(S, k):
    """(ids [nq, k] int32, scores [nq, k] f32) of a search whose score matrix is S [nq, n_docs]: larger first, equal scores (==) by
    smaller id, NaN never, -1 / -inf in the slots beyond"""
    S = np.asarray(S, dtype=np.float32).reshape(len(S), -1)
    if S.shape[1] == 0:
        return np.full((len(S), k), -1, np.int32), np.full((len(S), k), -np.inf, np.float32)
    return tor.reference_topk(S, np.ones(S.shape[1], dtype=bool), k)


def rescore_expected(S, cand, k):
    """a rescore of cand [nq, n_cand] under S: an id outside [0, n_docs) is no candidate, a repeated id as many candidates"""
    S = np.asarray(S, dtype=np.float32)
    cand = np.asarray(cand, dtype=np.int64)
    nq, n = cand.shape[0], S.shape[1]
    ids = np.full((nq, k), -1, np.int32)
    sc = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        c = cand[q][(cand[q] >= 0) & (cand[q] < n)]
        c = c[~np.isnan(S[q, c])]
        order = np.lexsort((c, -S[q, c].astype(np.float64)))[:k]
        ids[q, :len(order)] = c[order]
        sc[q, :len(order)] = S[q, c[order]]
    return ids, sc


def same_result(got, want):
    """ids equal; scores == and, where not zero, equal in bits (the sign of a zero is not promised)"""
    gi, gs = got
    wi, ws = want
    gs, ws = np.ascontiguousarray(gs, dtype=np.float32), np.ascontiguousarray(ws, dtype=np.float32)
    if not np.array_equal(gi, wi):
        return False
    nz = ws != 0
    return bool(np.array_equal(gs[nz].view(np.uint32), ws[nz].view(np.uint32)) and (gs[~nz] == 0).all())


def documents(rng, n_docs, dim, lens=DOC_LENS):
    """(rows f32 [., dim], cu int32): n_docs documents of unit rows whose lengths cycle through lens"""
    rows, cu, _ = mr.packed_set(rng, [lens[i % len(lens)] for i in range(n_docs)], dim)
    return rows, cu


def queries(rng, dim, lens=QUERY_LENS):
    """(rows, cu) of the lens that a search takes at this dim"""
    rows, cu, _ = mr.packed_set(rng, [n for n in lens if n <= max_query_tokens(dim)], dim)
    return rows, cu
