"""Two kernels have loops whose trip count depends on the size of the LAUNCH, not of a sentence; the other op-level tests are small and run
those loops once.  Here they run as the shipped shapes run them, and every test asserts through the geometry hooks
(bert_hip_test_sparse_vocab_geometry, bert_hip_test_attention_grid) that it reached the path it names — a retune of the slab rule or of
the grid rule fails these tests instead of leaving the loops uncovered.

sparse_vocab_kernel (sparse_vocab.hip): a wave's block loop runs slab_blocks / 8 rounds.  Slabs of 16, 24 and 64 (the cap) blocks, tile 64 at
16, a last slab of 2 and of 3 blocks (an odd count: one wave holds half a pair) — against float64 within sparse_bound, and bit-equal to
the same sentences served in pieces small enough for 8-block slabs, the path every other test checks.
attention_mfma_kernel<D, 512, 128> (attention.hip, the persistent form): a workgroup that walks four items with n_pad changing in both
directions; keys beyond 1024 tokens at d_head 32 (the second staging loop), alone and as a walked item; the launch limits, unlaunched.
Every case prints its geometry and its worst error / bound; profiles/launch_geometry_tests.txt records them."""
import functools

import numpy as np
import pytest

from bert_cpp_amd import pybert

import layer_reference as ref
import sparse_reference as sr
from attention_walk import _item_of, _walks          # noqa: F401  (the walk order, shared with the relative-position-bias tests)
from test_gpu_parity import _attention_ref
from test_gpu_sparse import _model_file, _op_inputs

pytestmark = pytest.mark.gpu

NAN16, NAN32 = 0x7E00, 0x7FC00000


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------
# 3a. the vocabulary kernel at op level
# ------------------------------------------------------------------------------------------------
# (H, V, T) -> the geometry at max_len 128 and the number of blocks in the last slab
SPARSE_CASES = [
    (64, 16421, 2048, dict(tile=128, n_tiles=16, slab_blocks=16, n_slabs=33), 2),
    (640, 16421, 1024, dict(tile=64, n_tiles=16, slab_blocks=16, n_slabs=33), 2),
    (64, 20001, 4096, dict(tile=128, n_tiles=32, slab_blocks=24, n_slabs=27), 2),
    (64, 28737, 8192, dict(tile=128, n_tiles=64, slab_blocks=64, n_slabs=15), 3),
]
SPARSE_LENS = [1, 31, 32, 33, 60, 68, 127, 128]


def _mixed_lens(T, seed):
    """a seeded mix of SPARSE_LENS that sums to T: sentences start and end inside sub-blocks, on tile edges and across them"""
    rng = np.random.default_rng(seed)
    lens = list(SPARSE_LENS)
    left = T - sum(lens)
    while left > 0:
        fit = [n for n in SPARSE_LENS if n <= left]
        lens.append(int(rng.choice(fit)))
        left -= lens[-1]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    assert sum(lens) == T and set(lens) == set(SPARSE_LENS)
    return lens


def _checked_columns(V, geo, seed):
    """the vocabulary columns held to float64: every column of the first and the last block of every slab, the whole last slab, and a
    seeded eighth of all columns"""
    nblk, sb = (V + 31) // 32, geo["slab_blocks"]
    blocks = set()
    for s in range(geo["n_slabs"]):
        blocks |= {s * sb, min((s + 1) * sb, nblk) - 1}
    blocks |= set(range((geo["n_slabs"] - 1) * sb, nblk))
    cols = np.zeros(V, dtype=bool)
    for b in blocks:
        cols[32 * b:32 * b + 32] = True
    cols[np.random.default_rng(seed).permutation(V)[:(V + 7) // 8]] = True
    cols[:2] = True
    return np.flatnonzero(cols)


def _float64_in_chunks(t, E, bias, lens, max_tokens=1024):
    """(sr.sparse, sr.sparse_bound with drows = 0) over runs of whole sentences of at most max_tokens tokens: no T x V matrix of doubles"""
    cu = _cu(lens)
    want, bound, b0 = [], [], 0
    while b0 < len(lens):
        b1 = b0 + 1
        while b1 < len(lens) and cu[b1 + 1] - cu[b0] <= max_tokens:
            b1 += 1
        rows = t[cu[b0]:cu[b1]]
        want.append(sr.sparse(rows, E, bias, lens[b0:b1]))
        bound.append(sr.sparse_bound(rows, 0.0, E, bias, lens[b0:b1], mfma=True))
        b0 = b1
    return np.concatenate(want), np.concatenate(bound)


@pytest.mark.parametrize("H,V,T,geometry,last_blocks", SPARSE_CASES, ids=[f"H{c[0]}-V{c[1]}-T{c[2]}" for c in SPARSE_CASES])
def test_vocabulary_kernel_beyond_one_round(H, V, T, geometry, last_blocks):
    """Slabs of more than 8 blocks: the later rounds of a wave (accumulators, fok / erow, the epilogue's atomic max again), a partial last
    slab, the cap at 64.  Worst error / bound measured on the MI355X: 3.3e-5 .. 5.2e-5 (the operands are f16 values, so only the f32
    accumulation and log1pf differ from float64); the bit comparison with the 8-block pieces is the sharp half."""
    lens = _mixed_lens(T, H + V)
    B, cu = len(lens), _cu(lens)
    geo = pybert.test_sparse_vocab_geometry(H, V, T, B, max(lens))
    print(f"sparse H {H} V {V} T {T} B {B}: geometry {geo}")
    assert geo == geometry, geo
    nblk = (V + 31) // 32
    assert nblk - (geo["n_slabs"] - 1) * geo["slab_blocks"] == last_blocks
    t, E, bias = _op_inputs(H, V, T)
    got = pybert.test_sparse_vocab(t, E, bias, cu, "mfma")
    assert got is not None and got.shape == (B, V)
    assert np.isfinite(got).all() and not np.signbit(got).any()
    assert (_bits(got[:, :2]) == 0).all()
    # float64, on the checked columns
    cols = _checked_columns(V, geo, T)
    assert len(cols) >= V / 8
    want, bound = _float64_in_chunks(t, E[cols], bias[cols], lens)
    err = np.abs(got[:, cols].astype(np.float64) - want)
    print(f"sparse H {H} V {V} T {T}: {len(cols)} of {V} columns, worst error / bound = {float((err / bound).max()):.3e}; "
          f"{float((got == 0).mean()):.3f} of the weights are zero")
    assert (err <= bound).all(), (H, V, T, float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())
    assert ((got[:, cols] == 0) == (want == 0)).mean() > 0.99
    # the same sentences in pieces whose slabs have 8 blocks: the same bits
    per_piece = max(n for n in range(1, 65) if pybert.test_sparse_vocab_geometry(H, V, T, n, 128)["slab_blocks"] == 8)
    for s0 in range(0, B, per_piece):
        ns = min(per_piece, B - s0)
        piece_geo = pybert.test_sparse_vocab_geometry(H, V, T, ns, max(lens[s0:s0 + ns]))
        assert piece_geo["slab_blocks"] == 8 and piece_geo["tile"] == geo["tile"], piece_geo
        piece = pybert.test_sparse_vocab(t, E, bias, cu, "mfma", s0=s0, ns=ns)
        assert _same(piece, got[s0:s0 + ns]), (H, V, T, s0, ns, np.argwhere(_bits(piece) != _bits(got[s0:s0 + ns]))[:5].tolist())


# ------------------------------------------------------------------------------------------------
# 3b. sparse, end to end
# ------------------------------------------------------------------------------------------------
def test_sparse_end_to_end_at_the_slab_cap(model_dir):
    """minilm-l6 with the MLM head (V = 30 522) on 64 x 128 tokens — slabs of 64 blocks, four rounds a wave — and on a ragged batch of
    about 8 200 tokens: finite non-negative rows, a sentence's row has the bits it has alone, top-k is the rule on the dense rows."""
    hp = sr.DIMS["minilm-l6"]
    m = pybert.BertModel(_model_file(model_dir, "minilm-l6", "f16"))
    rng = np.random.default_rng(64)
    ragged = [int(n) for n in rng.integers(1, 129, size=127)]
    ragged[0], ragged[-1] = 128, 1
    for name, lens in (("64 x 128", [128] * 64), ("ragged", ragged)):
        geo = pybert.test_sparse_vocab_geometry(hp.n_embd, hp.n_vocab, sum(lens), len(lens), max(lens))
        print(f"sparse end to end {name}: {sum(lens)} tokens, {len(lens)} sentences, geometry {geo}")
        assert geo["slab_blocks"] == 64 or name == "ragged", geo
        toks, cu, sents = sr.batch(rng, hp, lens)
        dense = m.sparse_packed(toks, cu)
        assert dense.shape == (len(lens), hp.n_vocab) and np.isfinite(dense).all() and (dense >= 0).all() and not np.signbit(dense).any()
        print(f"sparse end to end {name}: {float((dense == 0).mean()):.3f} of the weights are zero")
        others = rng.permutation(np.arange(1, len(lens) - 1))[:6]
        for b in [0, len(lens) - 1] + [int(b) for b in others]:
            alone = m.sparse_packed(sents[b], _cu([lens[b]]))
            assert _same(alone[0], dense[b]), (name, b, lens[b])
        for k in (10, 256):
            ids, wt = m.sparse_packed(toks, cu, k)
            want_ids, want_w = sr.topk(dense, k)
            assert np.array_equal(ids, want_ids) and _same(wt, want_w), (name, k)
    m.close()


# ------------------------------------------------------------------------------------------------
# 3c, 3d. attention: the persistent walk and long keys
# ------------------------------------------------------------------------------------------------
def _qkv(lens, n_head, d_head, seed):
    """test_attention_kernel's values: Q times 1.7, a dominant last key per sentence"""
    rng = np.random.default_rng(seed)
    cu = _cu(lens)
    H = n_head * d_head
    qkv = rng.normal(0, 1, (int(cu[-1]), 3 * H)).astype(np.float16)
    qkv[:, :H] *= 1.7
    for b in range(len(lens)):
        qkv[cu[b + 1] - 1, H:2 * H] *= 4.0
    return qkv, cu


def _clean_and_poisoned(qkv, cu, n_head, d_head):
    """the launch with zeros and with quiet NaNs in the padding rows and the output: the same bits, no NaN"""
    got = pybert.test_attention(qkv, cu, n_head, d_head, 0)
    with pybert.test_pad(NAN16, NAN32):
        dirty = pybert.test_attention(qkv, cu, n_head, d_head, 0)
    assert np.isfinite(got).all() and np.isfinite(dirty).all()
    assert _same(dirty, got), np.unique(np.argwhere(_bits(dirty) != _bits(got))[:, 0])[:8].tolist()
    return got


def _worst_fraction(got, qkv, cu, n_head, d, items):
    """the items (sentence n_head + head) against float64 within layer_reference.softmax_bound: the worst error / bound"""
    H, worst = n_head * d, 0.0
    for it in items:
        b, h = divmod(int(it), n_head)
        rows, sl = slice(cu[b], cu[b + 1]), slice(h * d, (h + 1) * d)
        bound, want = ref.softmax_bound(qkv[rows, sl], qkv[rows, H + h * d:H + (h + 1) * d], qkv[rows, 2 * H + h * d:2 * H + (h + 1) * d], 1 / np.sqrt(d))
        err = np.abs(ref.f8(got[rows, sl]) - want)
        assert (err <= bound).all(), (b, h, int(cu[b + 1] - cu[b]), float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())
        worst = max(worst, float((err / bound).max()))
    return worst


WALK_LENS = [1, 17, 128, 129, 130, 200, 257, 300, 384, 512]


def _attention_walk(d_head, n_head):
    _, cus, _ = pybert.test_attention_grid(4096, n_head, d_head, 512)      # (more items than any device has CUs: the grid is the CU rule's)
    B = next(b for b in range(1, 4096) if b * n_head >= 3 * cus + 8 and (b * n_head) % 8)
    rng = np.random.default_rng(1000 * d_head + n_head)
    lens = [512] + [int(n) for n in rng.choice(WALK_LENS, size=B - 1)]
    threads, grid, items = pybert.test_attention_grid(B, n_head, d_head, max(lens))
    walks = _walks(grid, items)
    print(f"attention walk d_head {d_head} n_head {n_head}: {B} sentences, {sum(lens)} tokens, threads {threads}, grid {grid}, items {items}, "
          f"a workgroup walks {min(map(len, walks))} .. {max(map(len, walks))} items")
    assert threads == 512 and grid == cus and items == B * n_head and items > 3 * grid and max(map(len, walks)) >= 4
    # consecutive items of a workgroup change n_pad in both directions
    pads = [[(lens[i // n_head] + 127) // 128 for i in w] for w in walks]
    assert any(a < b for p in pads for a, b in zip(p, p[1:])) and any(a > b for p in pads for a, b in zip(p, p[1:]))
    qkv, cu = _qkv(lens, n_head, d_head, sum(lens) + d_head)
    got = _clean_and_poisoned(qkv, cu, n_head, d_head)
    # float64: the derived bound on a seeded eighth of the items and on all items of two workgroups (one of them walks the most), the
    # rest to test_attention_kernel's 6e-3
    longest = max(range(grid), key=lambda g: len(walks[g]))
    bounded = set(int(i) for i in rng.permutation(items)[:items // 8]) | set(walks[longest]) | set(walks[grid - 1])
    worst = _worst_fraction(got, qkv, cu, n_head, d_head, sorted(bounded))
    err = np.abs(got.astype(np.float64) - _attention_ref(qkv, cu, n_head, d_head))
    print(f"attention walk d_head {d_head} n_head {n_head}: worst error / bound = {worst:.3f} over {len(bounded)} items "
          f"(workgroups {longest} and {grid - 1} whole); largest error of all {float(err.max()):.3e}")
    assert err.max() < 6e-3, (float(err.max()), np.argwhere(err > 6e-3)[:5].tolist())
    # a launch without a walk: groups of sentences with one workgroup per item, the wide form
    per_group = max(g for g in range(2, 17) if g * n_head <= cus and (g * n_head) % 8 == 0)
    for b0 in list(range(0, B - per_group, per_group)) + [B - per_group]:
        b1 = b0 + per_group
        assert max(lens[b0:b1]) > 128
        assert pybert.test_attention_grid(per_group, n_head, d_head, max(lens[b0:b1])) == (512, per_group * n_head, per_group * n_head)
        part = pybert.test_attention(qkv[cu[b0]:cu[b1]], _cu(lens[b0:b1]), n_head, d_head, 0)
        assert _same(part, got[cu[b0]:cu[b1]]), (b0, np.unique(np.argwhere(_bits(part) != _bits(got[cu[b0]:cu[b1]]))[:, 0])[:8].tolist())


def test_attention_walk_d32():
    """d_head 32, 12 heads: more than three items per workgroup of the persistent form — the next item's request under the mat-muls, the
    barrier between items, K / V^T re-laid in LDS as n_pad changes, the hand-over — against float64, bit-equal to launches of one item per
    workgroup and under NaN padding.  Measured on the MI355X (256 CUs: 780 items, 3 or 4 per workgroup): worst error / bound 0.376."""
    _attention_walk(32, 12)


def test_attention_walk_d64():
    """The same at d_head 64, 12 heads.  Measured: worst error / bound 0.341."""
    _attention_walk(64, 12)


# attention_mfma_grid takes d_head 32 up to 1152 tokens: n_pad 1152 needs 147 712 bytes of LDS, n_pad 1280 (1153 tokens and more) 164 096,
# above the 160 KiB (163 840 bytes) a workgroup can have
LONGEST_32 = 1152


@functools.lru_cache(maxsize=1)
def _companion():
    return np.random.default_rng(129).normal(0, 1, (129, 3 * 3 * 32)).astype(np.float16)


def _long_keys(lens, n_head, want_grid):
    d = 32
    H = n_head * d
    threads, grid, items = pybert.test_attention_grid(len(lens), n_head, d, max(lens))
    walks = _walks(grid, items)
    walked = [lens[i // n_head] for w in walks for i in w[1:]]
    print(f"attention long keys {lens} n_head {n_head}: threads {threads}, grid {grid}, items {items}, tokens of the walked items {walked}")
    assert (threads, grid, items) == (512, want_grid, len(lens) * n_head) and max(lens) > 1024
    qkv, cu = _qkv(lens, n_head, d, sum(lens))
    got = _clean_and_poisoned(qkv, cu, n_head, d)
    worst = _worst_fraction(got, qkv, cu, n_head, d, range(items))
    print(f"attention long keys {lens} n_head {n_head}: worst error / bound = {worst:.3f}")
    # each sentence beside one companion of 129 tokens, one workgroup per item
    comp = np.concatenate([_companion()[:, j * 3 * d:j * 3 * d + H] for j in range(3)], axis=1)
    for b, n in enumerate(lens):
        assert pybert.test_attention_grid(2, n_head, d, max(n, 129)) == (512, 2 * n_head, 2 * n_head)
        pair = pybert.test_attention(np.concatenate([qkv[cu[b]:cu[b + 1]], comp]), _cu([n, 129]), n_head, d, 0)
        assert _same(pair[:n], got[cu[b]:cu[b + 1]]), (b, n, np.unique(np.argwhere(_bits(pair[:n]) != _bits(got[cu[b]:cu[b + 1]]))[:, 0])[:8].tolist())
    return walked


def test_attention_long_keys_without_a_walk():
    """d_head 32, sentences of 1025, 600 and 1152 tokens (the longest the launcher takes), 2 heads: 6 items on a grid of 6.  The online
    softmax over 5 to 9 chunks, and the second staging loop (more than 2048 16-byte pieces of K / V: beyond 1024 tokens).  Measured: worst
    error / bound 0.221."""
    assert _long_keys([1025, 600, LONGEST_32], 2, 6) == []


def test_attention_long_keys_walked():
    """18 items on a grid of 16: the two walking workgroups take a second item, and one of those has more than 1024 tokens — its rows
    were requested under the first item's mat-muls and the second staging loop re-requests into those registers.  Measured: worst
    error / bound 0.354."""
    walked = _long_keys([LONGEST_32, 129, 1025, 7, 1100, 513], 3, 16)
    assert len(walked) == 2 and max(walked) > 1024


# ------------------------------------------------------------------------------------------------
# 3e. the launch limits, without a launch
# ------------------------------------------------------------------------------------------------
def test_attention_launch_limits():
    """The LDS limit of 160 KiB: d_head 32 up to 1152 tokens, d_head 64 up to 512; no other d_head.  The entry refuses what the grid hook
    refuses."""
    grid = lambda d, n: pybert.test_attention_grid(3, 2, d, n)
    for d, n in ((32, LONGEST_32 + 1), (32, 1216), (32, 1217), (64, 513), (48, 64), (48, 512)):
        assert grid(d, n) == (0, 0, 0), (d, n)
    assert grid(32, LONGEST_32) == (512, 6, 6) and grid(64, 512) == (512, 6, 6)
    assert grid(32, 128) == (256, 6, 6) and grid(64, 129) == (512, 6, 6)
    qkv = np.zeros((1217, 3 * 32), dtype=np.float16)
    with pytest.raises(RuntimeError, match="-2"):
        pybert.test_attention(qkv, _cu([1217]), 1, 32, 0)
    with pytest.raises(RuntimeError, match="-2"):
        pybert.test_attention(qkv[:LONGEST_32 + 1], _cu([LONGEST_32 + 1]), 1, 32, 0)
