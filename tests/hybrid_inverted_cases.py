"""The cells of the hybrid search over the postings (bert_hip.h "Hybrid search", "Over the postings"), shared by
tests/test_hybrid_inverted_host.py — which takes every cell's plan from the library's own hooks and asserts what the cell is there to
reach — and tests/test_gpu_hybrid_inverted.py, which runs them.  Also a NumPy model of where the scan reads a row's dense score, right
and wrong in three ways, with which the host file shows that the fixtures can tell.  No GPU, no library: the hooks are passed in."""
import numpy as np

import hybrid_reference as href
import index_reference as ixr
import sparse_index_reference as sref
import sparse_inverted_cases as cases
import topk_order_reference as tor

DENSE = ixr.DTYPES
SPARSE = ["f32", "f16"]
SEG_DEFAULT = cases.SEG_DEFAULT

# 1. random rows: 700 rows are three segments of 256, the last of 188 rows, or one partial segment of the default size; 33 queries are
# hybrid chunks of 32 + 1
R_ROWS, R_DIM, R_WIDTH, R_V, R_KQ = 700, 64, 16, 1000, 16
R_NQS = (1, 5, 33)
R_KS = (1, 10, 256)
R_SEGS = (cases.SEG_TEST, 0)                     # 0: the default
R_WEIGHTS = (0.7, 0.3)
R_MODES = ("plain", "dense removed", "sparse removed", "allow", "all three")

# 2. ordered and exact-fit scores: tor.hybrid_split_fixture, 4000 rows — one segment of 4096, or 15 segments of 256 and one of 160
O_KS = (1, 128, 129, 256)
O_SEGS = (tor.INVERTED_ONE_SEG, cases.SEG_TEST)
O_NQS = {tor.INVERTED_ONE_SEG: tor.HYBRID_NQS, cases.SEG_TEST: (3, 609)}      # 609: see check_ordered_plan
O_WALKED_NQ = 609

# 3. the 34 816-row fixture of tests/test_gpu_hybrid_order.py: 17 segments of the default size, one per slice
M_NQS = tor.MANY_NQS
M_KS = tor.MANY_KS
M_CHUNK_NQ, M_CHUNK = 5, 2

_CACHE = {}


def seg_of(seg):
    return seg or SEG_DEFAULT


def plan(chunk_hook, geo_hook, sd, n_vocab, n_rows, nq, k, seg, qb=0, pref=0):
    """([(c0, c, g)], ld): the hybrid chunks of a call (chunk_hook = pybert.test_hybrid_chunk) and each chunk's postings geometry
    (geo_hook = pybert.test_sparse_postings_geometry) with seg, n_segs and slice_rows added — what Hybrid::search_device itself calls"""
    seg = seg_of(seg)
    chunks, ld = tor.hybrid_chunks(n_rows, nq, pref, chunk_hook)
    out = []
    for c0, c in chunks:
        g = dict(geo_hook(SPARSE.index(sd), n_vocab, n_rows, c, k, seg, qb))
        g["seg"], g["n_segs"], g["slice_rows"] = seg, -(-n_rows // seg), g["slice_segs"] * seg
        assert g["n_slices"] <= g["max_slices"] and g["lds"] <= 160 * 1024 - 256, g
        out.append((c0, c, g))
    return out, ld


def check_random_plan(p, seg, nq):
    """700 rows: a partial last segment always; three one-segment slices at 256; 33 queries: a second chunk of one query"""
    chunks, ld = p
    g = chunks[0][2]
    assert ld == 704 and R_ROWS % g["seg"] not in (0,) and R_ROWS % g["seg"] % 64 != 0, g
    if seg_of(seg) == cases.SEG_TEST:
        assert g["n_segs"] == 3 and R_ROWS - 2 * cases.SEG_TEST == 188 and g["n_slices"] == 3, g
    else:
        assert g["n_segs"] == 1 and g["n_slices"] == 1, g
    assert [(c0, c) for c0, c, _ in chunks] == ([(0, 32), (32, 1)] if nq == 33 else [(0, nq)]), chunks


def check_ordered_plan(p, seg, nq, n_rows=tor.SPARSE_ROWS):
    """seg 4096: one partial segment.  seg 256: every step is a segment edge and the last segment has 160 rows; 609 queries are a chunk
    of 608 — 304 tiles of two, whose workgroups walk slices of 3 segments, the last slice being the partial segment alone — and a
    second chunk of one query, one segment a slice"""
    chunks, ld = p
    g = chunks[0][2]
    assert ld == 4032 and n_rows % g["seg"] != 0, g
    if seg == tor.INVERTED_ONE_SEG:
        assert g["n_segs"] == 1 and g["n_slices"] == 1 and len(chunks) == 1 and g["qb"] == min(2, nq), g
        return
    assert g["n_segs"] == 16 and n_rows - 15 * 256 == 160, g
    if nq == O_WALKED_NQ:
        assert [(c0, c) for c0, c, _ in chunks] == [(0, 608), (608, 1)], chunks
        assert g["qb"] == 2 and g["n_qtiles"] == 304 and g["slice_segs"] >= 3 and g["n_slices"] > 1, g
        last = (g["n_slices"] - 1) * g["slice_segs"]
        assert last <= g["n_segs"] - 1 < last + g["slice_segs"], g                     # the partial segment ends the last slice
        g1 = chunks[1][2]
        assert g1["qb"] == 1 and g1["slice_segs"] == 1 and g1["n_slices"] == 16, g1
    else:
        assert len(chunks) == 1 and g["qb"] == 2 and g["slice_segs"] == 1 and g["n_slices"] == 16, g


def check_many_plan(p, nq, pref=0):
    """34 816 rows: 17 whole segments of 2048, every one a slice; row r's dense score lies r floats into its query's line of the score
    matrix, for 16 of the 17 slices beyond the slice's own length"""
    chunks, ld = p
    assert ld == tor.MANY_SPARSE_ROWS == 17 * SEG_DEFAULT
    for _, _, g in chunks:
        assert g["n_segs"] == 17 and g["n_slices"] == 17 and g["slice_segs"] == 1, g
    if pref:
        assert [(c0, c) for c0, c, _ in chunks] == [(0, 2), (2, 2), (4, 1)], chunks
    elif nq == 33:
        assert [(c0, c) for c0, c, _ in chunks] == [(0, 32), (32, 1)], chunks
    else:
        assert len(chunks) == 1


# ------------------------------------------------------------------------------------------------
# the random case's data and references
# ------------------------------------------------------------------------------------------------
def random_data():
    """(dense rows, dense queries, term ids, term weights, query ids, query weights), made once"""
    if "random" not in _CACHE:
        rng = np.random.default_rng(715)
        rows = ixr.unit(rng.standard_normal((R_ROWS, R_DIM)))
        queries = ixr.unit(rng.standard_normal((max(R_NQS), R_DIM)))
        ids, w = cases._terms(rng, R_ROWS, R_WIDTH, R_V, R_WIDTH, 2.0)
        q_ids, q_w = cases._terms(rng, max(R_NQS), R_KQ, R_V, R_KQ, 2.0)
        out = (rows, queries, ids, w, q_ids, q_w)
        for a in out:
            a.setflags(write=False)
        _CACHE["random"] = out
    return _CACHE["random"]


def random_sparse_scores(sd):
    """S [33][700] of the stored rows by sparse_index_reference, made once"""
    if ("S", sd) not in _CACHE:
        _, _, ids, w, q_ids, q_w = random_data()
        st = sref.stored_rows(ids, w, R_WIDTH, sd)
        S = sref.scores(st[0], st[1], q_ids, q_w, R_V)
        S.setflags(write=False)
        _CACHE[("S", sd)] = S
    return _CACHE[("S", sd)]


def random_masks():
    """(rows removed from the dense index, rows removed from the sparse index, the allow-list) — each takes rows of every segment,
    the last one's tail included"""
    rng = np.random.default_rng(9)
    gone_d = np.sort(rng.permutation(R_ROWS)[:150]).astype(np.int32)
    gone_s = np.sort(rng.permutation(R_ROWS)[:150]).astype(np.int32)
    allow = rng.random(R_ROWS) < 0.5
    for a in (gone_d, gone_s, np.flatnonzero(~allow)):
        assert (a < 256).any() and (a >= 512).any() and (a >= R_ROWS - 60).any()
    return gone_d, gone_s, allow


def random_mode(mode):
    """(gone_d, gone_s, allow or None, the rows that qualify) of one of R_MODES"""
    gone_d, gone_s, allow = random_masks()
    none = np.zeros(0, np.int32)
    gd = gone_d if mode in ("dense removed", "all three") else none
    gs = gone_s if mode in ("sparse removed", "all three") else none
    al = allow if mode in ("allow", "all three") else None
    qual = np.ones(R_ROWS, bool)
    qual[gd] = False
    qual[gs] = False
    if al is not None:
        qual &= al
    return gd, gs, al, qual


# ------------------------------------------------------------------------------------------------
# where the scan reads D: a model, right and wrong
# ------------------------------------------------------------------------------------------------
READS = ("global row, chunk query", "row inside the segment", "row inside the slice", "query of the call")


def model_search(D, S, qual, wd, ws, k, p, read=READS[0]):
    """hybrid_reference.search over the D the scan would read under the plan p = plan(...): the score matrix holds the current chunk's
    queries in its first lines ([c][ld]; behind them whatever earlier chunks left, +0 at first) and row r's score at column r.  The
    right read is line (query inside the chunk), column (global row).  The three wrong reads take the column inside the segment, the
    column inside the slice, or the line of the query's index in the call."""
    assert read in READS
    chunks, ld = p
    nq, n = D.shape
    buf = np.zeros((max(nq, chunks[0][1]), ld), np.float32)
    Dr = np.empty((nq, n), np.float32)
    rows = np.arange(n)
    for c0, c, g in chunks:
        buf[:c, :n] = D[c0:c0 + c]
        col = {READS[1]: rows % g["seg"], READS[2]: rows % g["slice_rows"]}.get(read, rows)
        for q in range(c):
            Dr[c0 + q] = buf[c0 + q if read == READS[3] else q, col]
    return href.search(Dr, S, qual, wd, ws, k)
