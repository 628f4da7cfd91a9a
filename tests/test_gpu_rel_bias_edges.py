"""GPU tests of the relative position bias at its structural edges — what test_gpu_rel_bias.py's one launch shape (14 lengths up to 512 in
one batch, 2 heads, P = 512, W ~ N(0, 2^2)) cannot see:

  A.1  keys beyond 512 tokens at d_head 32: the strided loop of the table staging (attention.hip: the 1024 prefetched entries hold the
       window of at most 512 tokens), alone, beside a companion, with NaN outside the window and in the padding;
  A.2  walked launches whose table moves: consecutive items of a workgroup with a larger and with a smaller n_pad, onto an item of more
       than 1024 tokens;
  A.3  the deep walk of test_gpu_launch_geometry.py with a bias;
  A.4  the result does not depend on P;      A.5  a sentence alone = in the batch with W != 0;
  A.6  hard values: the lookup alone (Q = 0), maxima that move by 300 through the bias alone, a loud table;
  A.7  the generic kernel where the engine needs it (d_head 20 and 96; 65 537 sentences: the second slice of the launchers);
  A.8  the launch limits;
  B    end to end: alone = in the batch per model, and five models at the table lengths, routes and d_heads the suite had not loaded.

References and bounds are rel_bias_reference.py's; the walk order is attention_walk.py's.  Every case prints its geometry and its worst
error / bound; profiles/rel_bias_edges.txt is the -s output of the committed run."""
import os

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import rel_bias_reference as rb
from attention_walk import _walks, walk_lengths
from test_gpu_launch_geometry import WALK_LENS
from test_gpu_rel_bias import _launches, e2e_file

pytestmark = pytest.mark.gpu

NAN16, NAN32 = 0x7E00, 0x7FC00000
IMPL = {"mfma": 0, "naive": 1}
KINDS = ("mfma", "naive", "f32")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _rows_that_differ(a, b):
    return np.unique(np.argwhere(_bits(a) != _bits(b))[:, 0])[:8].tolist()


def _run(kind, qkv, lens, n_head, d_head, W, P, rel=None):
    """the kernel `kind` on packed sentences of `lens`: f16 rows for the two f16 kernels, f32 rows for the f32 one"""
    if kind == "f32":
        return pybert.test_f32_attention_bias(np.asarray(qkv, dtype=np.float32), rb.cu_of(lens), n_head, d_head, max(lens), W, P)
    return pybert.test_attention_bias(qkv, rb.cu_of(lens), n_head, d_head, IMPL[kind], W, P, rel=rel)


def _run_padded(kind, qkv, lens, n_head, d_head, W, P, rel=None):
    with pybert.test_pad(NAN16, NAN32):
        return _run(kind, qkv, lens, n_head, d_head, W, P, rel)


def _fractions(got, want, bnd, lens):
    """the worst error / bound per sentence, in order"""
    cu = rb.cu_of(lens)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(got.astype(np.float64) - want) / bnd
    return [float(frac[cu[b]:cu[b + 1]].max()) for b in range(len(lens))]


def _within(frac):
    """every fraction is at most 1 (a NaN is not)"""
    return bool((np.asarray(frac) <= 1.0).all())


def _alone(kind, qkv, lens, b, n_head, d_head, W, P):
    cu = rb.cu_of(lens)
    return _run(kind, qkv[cu[b]:cu[b + 1]], [lens[b]], n_head, d_head, W, P)


def _poisoned_table(W, P, n, d_head, kind):
    """the table the kernel `kind` takes (the matrix cores: times sqrt(d_head), rounded once), NaN outside a sentence of n tokens' window"""
    table = (rb.rel_table(W, P).astype(np.float64) * (np.sqrt(d_head) if kind == "mfma" else 1.0)).astype(np.float32)
    out = np.full_like(table, np.nan)
    out[:, P - n:P + n - 1] = table[:, P - n:P + n - 1]
    return out


# ------------------------------------------------------------------------------------------------
# A.1 long keys
# ------------------------------------------------------------------------------------------------
def test_long_keys_stage_the_whole_window():
    """d_head 32, P = 1152, sentences of 1152, 600 and 1025 tokens, 2 heads: 6 items on a grid of 6.  The table window has 2 n - 1 = 2303,
    1199 and 2049 entries; the first 1024 are prefetched, the rest is the strided loop no other test runs.  Within mfma_bound; each
    sentence beside a 129-token companion (one workgroup per item), with NaN outside its window and NaN padding: the same bits.
    Measured on the MI355X: worst error / bound 0.255 (1152 tokens), 0.286 (600), 0.269 (1025)."""
    d, nh, P, lens = 32, 2, rb.P_LONG, rb.LONG_LENS
    assert pybert.test_attention_grid(len(lens), nh, d, max(lens)) == (512, 6, 6)
    qkv, W, want, bnd = rb.reference(lens, nh, d, "mfma")
    got = _run("mfma", qkv, lens, nh, d, W, P)
    frac = _fractions(got, want, bnd, lens)
    print(f"\nlong keys d_head 32 P {P}: worst fraction of the bound per length {dict(zip(lens, np.round(frac, 3)))}")
    assert _within(frac), frac
    dirty = _run_padded("mfma", qkv, lens, nh, d, W, P)
    assert np.isfinite(got).all() and _same(dirty, got), _rows_that_differ(dirty, got)
    comp = rb.op_inputs((129,), nh, d)
    cu = rb.cu_of(lens)
    for b, n in enumerate(lens):
        rows = got[cu[b]:cu[b + 1]]
        assert pybert.test_attention_grid(2, nh, d, n) == (512, 2 * nh, 2 * nh)
        pair = _run("mfma", np.concatenate([qkv[cu[b]:cu[b + 1]], comp]), [n, 129], nh, d, W, P)
        assert _same(pair[:n], rows), (n, _rows_that_differ(pair[:n], rows))
        loud = _run_padded("mfma", qkv[cu[b]:cu[b + 1]], [n], nh, d, None, P, rel=_poisoned_table(W, P, n, d, "mfma"))
        assert not np.isnan(loud).any() and _same(loud, rows), (n, _rows_that_differ(loud, rows))


# ------------------------------------------------------------------------------------------------
# A.2 walked launches whose table moves
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_head", [32, 64])
def test_a_walk_moves_the_table(d_head):
    """13 sentences, 2 heads: 26 items on a grid of 24, workgroups 0 and 1 take a second item.  The table lies behind K and V^T at an
    offset that depends on the item's own n_pad: 512 -> 5 tokens moves it down (into what was K), 7 -> 1152 (d_head 32; 400 at d_head
    64) moves it up, and at d_head 32 the second item's window needs the strided loop.  All items within mfma_bound; NaN padding and
    every sentence launched alone: the same bits.  Measured: worst error / bound 0.464 at d_head 32 (the 5 tokens behind 512),
    0.404 at d_head 64 (the 7 tokens in front of 400); the walked 1152 tokens 0.228."""
    nh = 2
    P, lens = rb.MOVING_WALK[d_head]
    threads, grid, items = pybert.test_attention_grid(len(lens), nh, d_head, max(lens))
    walked = [w for w in walk_lengths(lens, nh, grid) if len(w) > 1]
    print(f"\nmoving walk d_head {d_head} P {P}: threads {threads}, grid {grid}, items {items}, tokens along the walks {walked}")
    assert threads == 512 and items == len(lens) * nh and grid < items
    pads = [[(n + 127) // 128 for n in w] for w in walked]
    assert len(walked) >= 2 and any(p[1] > p[0] for p in pads) and any(p[1] < p[0] for p in pads)
    assert d_head != 32 or any(n > 1024 for w in walked for n in w[1:])
    qkv, W, want, bnd = rb.reference(lens, nh, d_head, "mfma")
    got = _run("mfma", qkv, lens, nh, d_head, W, P)
    frac = _fractions(got, want, bnd, lens)
    print(f"moving walk d_head {d_head}: worst fraction of the bound per sentence {dict(zip(lens, np.round(frac, 3)))}")
    assert _within(frac), frac
    dirty = _run_padded("mfma", qkv, lens, nh, d_head, W, P)
    assert np.isfinite(got).all() and _same(dirty, got), _rows_that_differ(dirty, got)
    cu = rb.cu_of(lens)
    for b, n in enumerate(lens):
        one = _alone("mfma", qkv, lens, b, nh, d_head, W, P)
        assert _same(one, got[cu[b]:cu[b + 1]]), (b, n, _rows_that_differ(one, got[cu[b]:cu[b + 1]]))


# ------------------------------------------------------------------------------------------------
# A.3 the deep walk
# ------------------------------------------------------------------------------------------------
def _deep_walk(d_head, n_head=12, P=512):
    _, cus, _ = pybert.test_attention_grid(4096, n_head, d_head, 512)      # (more items than any device has CUs: the grid is the CU rule's)
    B = next(b for b in range(1, 4096) if b * n_head >= 3 * cus + 8 and (b * n_head) % 8)
    rng = np.random.default_rng(2000 * d_head + n_head)
    lens = tuple([512] + [int(n) for n in rng.choice(WALK_LENS, size=B - 1)])
    threads, grid, items = pybert.test_attention_grid(B, n_head, d_head, max(lens))
    walks = _walks(grid, items)
    print(f"\ndeep walk with a bias d_head {d_head} n_head {n_head}: {B} sentences, {sum(lens)} tokens, threads {threads}, grid {grid}, "
          f"items {items}, a workgroup walks {min(map(len, walks))} .. {max(map(len, walks))} items")
    assert threads == 512 and grid == cus and items == B * n_head and items > 3 * grid and max(map(len, walks)) >= 4
    pads = [[(lens[i // n_head] + 127) // 128 for i in w] for w in walks]
    assert any(a < b for p in pads for a, b in zip(p, p[1:])) and any(a > b for p in pads for a, b in zip(p, p[1:]))
    qkv, W = rb.op_inputs(lens, n_head, d_head), rb.draw_W(n_head)
    got = _run("mfma", qkv, lens, n_head, d_head, W, P)
    dirty = _run_padded("mfma", qkv, lens, n_head, d_head, W, P)
    assert np.isfinite(got).all() and _same(dirty, got), _rows_that_differ(dirty, got)
    # float64: the derived bound on a seeded eighth of the items and on all items of the longest-walking workgroup and of the last one
    longest = max(range(grid), key=lambda g: len(walks[g]))
    bounded = set(int(i) for i in rng.permutation(items)[:items // 8]) | set(walks[longest]) | set(walks[grid - 1])
    want, bnd = rb.attention_packed(qkv, lens, n_head, d_head, W, "mfma", items=bounded)
    cu, worst = rb.cu_of(lens), 0.0
    for it in sorted(bounded):
        b, h = divmod(it, n_head)
        rows, sl = slice(cu[b], cu[b + 1]), slice(h * d_head, (h + 1) * d_head)
        frac = float((np.abs(got[rows, sl].astype(np.float64) - want[rows, sl]) / bnd[rows, sl]).max())
        assert frac <= 1.0, (b, h, lens[b], frac)
        worst = max(worst, frac)
    print(f"deep walk with a bias d_head {d_head}: worst error / bound = {worst:.3f} over {len(bounded)} items (workgroups {longest} and {grid - 1} whole)")
    # launches without a walk: groups of sentences with one workgroup per item
    per_group = max(g for g in range(2, 17) if g * n_head <= cus and (g * n_head) % 8 == 0)
    for b0 in list(range(0, B - per_group, per_group)) + [B - per_group]:
        b1 = b0 + per_group
        assert max(lens[b0:b1]) > 128
        assert pybert.test_attention_grid(per_group, n_head, d_head, max(lens[b0:b1])) == (512, per_group * n_head, per_group * n_head)
        part = _run("mfma", qkv[cu[b0]:cu[b1]], lens[b0:b1], n_head, d_head, W, P)
        assert _same(part, got[cu[b0]:cu[b1]]), (b0, _rows_that_differ(part, got[cu[b0]:cu[b1]]))


def test_deep_walk_with_a_bias_d32():
    """test_gpu_launch_geometry.py's deep walk (more than three items per workgroup, 12 heads, n_pad changing in both directions) with
    W ~ N(0, 2^2): the table re-staged at a new offset for every item while the next item's K / V rows are in flight.  Measured (256 CUs: 780 items, 3 or 4 per workgroup): worst error /
    bound 0.371 over 104 items."""
    _deep_walk(32)


def test_deep_walk_with_a_bias_d64():
    """Measured: worst error / bound 0.377 over 102 items."""
    _deep_walk(64)


# ------------------------------------------------------------------------------------------------
# A.4 the result does not depend on P
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(rb.P_FREE))
@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_the_result_does_not_depend_on_the_table_length(kind, d_head, form):
    """The window starts at rel[h][P - n] and a head's row has the odd length 2 P - 1: one W, one batch, every P gives the same bits
    (the one-chunk form with n = P = 128 — the window is the whole row — and the persistent form)."""
    lens, Ps = rb.P_FREE[form]
    assert min(Ps) == max(lens)
    qkv, W = rb.op_inputs(lens, 2, d_head), rb.draw_W(2)
    if kind == "mfma":
        assert pybert.test_attention_grid(len(lens), 2, d_head, max(lens))[0] == (256 if form == "one chunk" else 512)
    first = _run(kind, qkv, lens, 2, d_head, W, Ps[0])
    assert np.isfinite(first).all()
    for P in Ps[1:]:
        other = _run(kind, qkv, lens, 2, d_head, W, P)
        assert _same(other, first), (P, _rows_that_differ(other, first))


@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_the_shortest_table(kind, d_head):
    """P = 128 with sentences of 1, 2, 127 and 128 tokens, within the kernel's bound.  Measured (d_head 32 / 64): matrix cores 0.366 /
    0.317, naive 0.477 / 0.458, f32 0.021 / 0.012."""
    lens = rb.P_SMALL_LENS
    qkv, W, want, bnd = rb.reference(lens, 2, d_head, kind)
    frac = _fractions(_run(kind, qkv, lens, 2, d_head, W, 128), want, bnd, lens)
    print(f"\nP 128 {kind} d_head {d_head}: worst fraction of the bound per length {dict(zip(lens, np.round(frac, 3)))}")
    assert _within(frac), frac


# ------------------------------------------------------------------------------------------------
# A.5 alone = in the batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_a_sentence_alone_has_its_bits_of_the_batch(kind, d_head):
    """DESIGN §5's promise with W != 0: alone, a sentence of up to 128 tokens runs the 4-wave form, in the batch of LENS the persistent one"""
    lens, P = rb.LENS, rb.P_OP
    qkv, W = rb.op_inputs(lens, 2, d_head), rb.draw_W(2)
    got = _run(kind, qkv, lens, 2, d_head, W, P)
    cu = rb.cu_of(lens)
    for b, n in enumerate(lens):
        one = _alone(kind, qkv, lens, b, 2, d_head, W, P)
        assert _same(one, got[cu[b]:cu[b + 1]]), (n, _rows_that_differ(one, got[cu[b]:cu[b + 1]]))


# ------------------------------------------------------------------------------------------------
# A.6 hard values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(rb.HARD_CASES))
@pytest.mark.parametrize("d_head", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_hard_values(kind, d_head, case):
    """rel_bias_reference.HARD_CASES, each kernel within its bound as it stands.  The matrix-core accumulators START from bias sqrt(d);
    in `rise` / `fall` the running maximum moves by 300 natural units twice between chunks through the bias alone.  No kernel leaves
    its bound and no bound was changed.  Measured worst error / bound (d_head 32 / 64):
                      lookup          rise            fall            loud
        matrix cores  0.385 / 0.448   0.274 / 0.264   0.283 / 0.254   0.273 / 0.265
        naive         0.496 / 0.497   0.442 / 0.418   0.458 / 0.436   0.476 / 0.458
        f32           0.082 / 0.113   0.188 / 0.121   0.134 / 0.121   0.082 / 0.051"""
    lens = rb.HARD_CASES[case]
    qkv, W, want, bnd = rb.reference(lens, 2, d_head, kind, case=case)
    got = _run(kind, qkv, lens, 2, d_head, W, rb.P_OP)
    assert np.isfinite(got).all()
    frac = _fractions(got, want, bnd, lens)
    print(f"\nhard values {case} {kind} d_head {d_head}: worst fraction of the bound per length {dict(zip(lens, np.round(frac, 3)))}")
    assert _within(frac), frac


# ------------------------------------------------------------------------------------------------
# A.7 the generic kernel where the engine needs it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_head", rb.GENERIC_D_HEADS)
def test_generic_kernel_at_other_head_widths(d_head):
    """d_head 20 and 96: no matrix-core kernel, the engine's attention is attention_naive_kernel with the unscaled table.  Measured: worst
    error / bound 0.484 (d_head 20), 0.444 (d_head 96)."""
    lens = rb.GENERIC_LENS
    assert pybert.test_attention_grid(len(lens), 2, d_head, max(lens)) == (0, 0, 0)
    qkv, W, want, bnd = rb.reference(lens, 2, d_head, "naive")
    frac = _fractions(_run("naive", qkv, lens, 2, d_head, W, rb.P_OP), want, bnd, lens)
    print(f"\nnaive d_head {d_head}: worst fraction of the bound per length {dict(zip(lens, np.round(frac, 3)))}")
    assert _within(frac), frac


@pytest.mark.parametrize("kind", ["naive", "f32"])
def test_the_second_slice_of_sentences(kind):
    """65 537 sentences of 2 tokens, 1 head of d_head 2: grid.y holds 65 535, the launcher's second slice starts at cu_seqlens + 65535
    with the same table.  Every row against float64 within the bound; the last sentence has the bits it has alone.  Measured: worst
    error / bound 0.499 (naive; 0.399 in the second slice) and 0.116 (f32; 0.050)."""
    qkv, W = rb.many_inputs(), rb.draw_W(1)
    lens = [2] * rb.MANY
    want, bnd = rb.many_reference(qkv.astype(np.float32) if kind == "f32" else qkv, W, kind)
    got = _run(kind, qkv, lens, 1, 2, W, rb.P_OP)
    frac = np.abs(got.astype(np.float64) - want) / bnd
    print(f"\n{rb.MANY} sentences {kind}: worst fraction of the bound {float(frac.max()):.3f}, in the second slice {float(frac[2 * 65535:].max()):.3f}")
    assert frac.max() <= 1.0, np.argwhere(frac > 1.0)[:5].tolist()
    one = _run(kind, qkv[-2:], [2], 1, 2, W, rb.P_OP)
    assert _same(one, got[-2:])


# ------------------------------------------------------------------------------------------------
# A.8 limits
# ------------------------------------------------------------------------------------------------
def test_launch_limits_with_a_bias():
    """The table's 8 n_pad bytes still fit where the launch without a bias fits (d_head 32: 156 928 of 163 840 bytes at 1152 tokens); one
    chunk more is refused with -2 as it is without a bias."""
    W = np.zeros((32, 1), dtype=np.float32)
    for d, n in ((32, 1152), (64, 512)):
        assert pybert.test_attention_grid(1, 1, d, n)[0] == 512
        out = pybert.test_attention_bias(np.zeros((n, 3 * d), dtype=np.float16), rb.cu_of([n]), 1, d, 0, W, n)
        assert out.shape == (n, d) and not out.any()
    for d, n in ((32, 1153), (64, 513)):
        assert pybert.test_attention_grid(1, 1, d, n) == (0, 0, 0)
        with pytest.raises(RuntimeError, match="-2"):
            pybert.test_attention_bias(np.zeros((n, 3 * d), dtype=np.float16), rb.cu_of([n]), 1, d, 0, W, n)


# ------------------------------------------------------------------------------------------------
# B. end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rb.E2E_MODELS))
def test_models_alone_is_in_the_batch(model_dir, name):
    """eval_packed of each sentence alone = its row of the batch, bit for bit, on the LAYERED, FOLDED and F32 routes"""
    m = pybert.BertModel(e2e_file(model_dir, name))
    sents = rb.e2e_sentences(name)
    got = m.eval_packed(np.concatenate(sents), rb.cu_of([len(s) for s in sents]))
    for b, s in enumerate(sents):
        one = m.eval_packed(s, rb.cu_of([len(s)]))
        assert _same(one[0], got[b]), (name, len(s), float(np.abs(one[0] - got[b]).max()))
    m.close()


# The tolerance on |row - float64| / max |row|, as in test_gpu_rel_bias.py: twice what the PARENT commit's library leaves on the same
# encoder weights WITHOUT the tensor against the float64 model with W = 0, on the same sentences and calls.  Measured on an MI355X by
#     python tools/rel_bias_parent.py --parent <bert.cpp_amd of a built parent checkout>       (profiles/rel_bias_edges_parent.txt)
# (Measured with the parent's library as it was; the run reproduced the ten figures and two digests of profiles/rel_bias_parent.txt
# to the last digit.  A file without the tensor runs the kernels without a bias, which this commit leaves as they were.)
PARENT_POOLED_ERROR = {"h64-p128-f16": 8.921e-04, "h64-p1152-f16": 7.974e-04, "h64-p1152-f32": 8.095e-07, "h128-p640-f16": 2.676e-04, "h80-f16": 7.228e-04}
PARENT_HIDDEN_ERROR = {"h64-p128-f16": 2.237e-03, "h64-p1152-f16": 2.126e-03, "h64-p1152-f32": 1.489e-06, "h128-p640-f16": 2.393e-03, "h80-f16": 2.081e-03}
EDGE_ROUTE = {"h64-p128-f16": "layered", "h64-p1152-f16": "layered", "h64-p1152-f32": "f32", "h128-p640-f16": "layered", "h80-f16": "layered"}


def edge_file(model_dir, name, rel_bias=True):
    hp, ftype, _ = rb.E2E_EDGE_MODELS[name]
    path = os.path.join(model_dir, f"relbias_edge_{name}_{int(rel_bias)}.bin")
    if not os.path.exists(path):
        gf.write_model(path, hp, gf.synthetic_weights(hp, rb.E2E_SEED, rel_bias=rel_bias), gf.FTYPE_BY_NAME[ftype])
    return path


def edge_errors(m, ref, calls):
    """(pooled error over the calls, hidden-state error over the distinct sentences, the rows of every call)"""
    hid, rows, e_pool = {}, [], []
    for sents in calls:
        for s in sents:
            if len(s) not in hid:
                hid[len(s)] = (s, ref.hidden(s))
        got = m.eval_packed(np.concatenate(sents), rb.cu_of([len(s) for s in sents]))
        last = [hid[len(s)][1][-1].mean(axis=0) for s in sents]
        e_pool.append(rb.row_error(got, np.stack([y / np.linalg.norm(y) for y in last])))
        rows.append(got)
    e_hid = {n: rb.row_error(m.eval_hidden(s)[1], h) for n, (s, h) in hid.items()}
    return float(np.max(e_pool)), e_hid, rows                 # (np.max: a NaN row is a NaN error, and fails every comparison)


@pytest.mark.parametrize("name", list(rb.E2E_EDGE_MODELS))
def test_edge_models_match_float64_end_to_end(model_dir, name):
    """rel_bias_reference.E2E_EDGE_MODELS against the float64 model: the pooled rows of every call and every layer's hidden states of
    every sentence, within twice the parent's error without the tensor.  Measured on the MI355X, pooled / hidden (allowed):
        h64-p128-f16   9.973e-04 / 2.550e-03  (1.784e-03 / 4.474e-03)      h64-p1152-f16  5.647e-04 / 2.861e-03  (1.595e-03 / 4.252e-03)
        h128-p640-f16  3.722e-04 / 2.653e-03  (5.352e-04 / 4.786e-03)      h80-f16        5.347e-04 / 1.775e-03  (1.446e-03 / 4.162e-03)
        h64-p1152-f32  7.706e-07 / 1.524e-06  (1.619e-06 / 2.978e-06)
    This test found something: with f32_attention_kernel as the feature shipped it, h64-p1152-f32 left 3.009e-06 in the hidden states
    at 1152 tokens, 1 % over its tolerance (600: 1.753e-06, 129: 1.519e-06).  The kernel summed P.V as ONE chain of n fused
    multiply-adds; a NumPy float32 forward of the file with that chain leaves 2.52e-06 with the table (1.31e-06 without: the table
    doubles what the chain loses), with four chains of n / 4 1.20e-06, and with NumPy's blocked mat-mul 1.54e-06.  The kernel with a
    bias now sums in four chains (f32_route.hip) and leaves 1.182e-06 at 1152 tokens; the kernel without one keeps its order."""
    path = edge_file(model_dir, name)
    ref = rb.Model(path)
    m = pybert.BertModel(path, test_routes=name == "h128-p640-f16")         # (the "attn" switch below lives in libbert_test.so)
    assert m.relative_attention
    calls = rb.edge_calls(name)
    rep = _launches(m, lambda: m.eval_packed(np.concatenate(calls[0]), rb.cu_of([len(s) for s in calls[0]])))
    assert rep.get("attention", 0) == ref.hp.n_layer and not any(k in rep for k in ("qkv_attention2", "model_kernel")), rep
    assert ("family:gemm_f32" in rep) == (EDGE_ROUTE[name] == "f32") and "ln_rows_finalize" not in rep, rep
    e_pool, e_hid, rows = edge_errors(m, ref, calls)
    print(f"\n{name}: pooled {e_pool:.3e} (parent {PARENT_POOLED_ERROR.get(name)}), hidden per length "
          f"{({n: float(f'{e:.3e}') for n, e in e_hid.items()})} (parent {PARENT_HIDDEN_ERROR.get(name)}); launches {rep}")
    assert e_pool <= 2 * PARENT_POOLED_ERROR[name] and float(np.max(list(e_hid.values()))) <= 2 * PARENT_HIDDEN_ERROR[name]
    if name == "h128-p640-f16":
        # the switch: beyond 512 tokens the matrix cores refuse d_head 64 and the call IS the generic kernel's; at 512 it is not
        m.set_option("attn", "naive")
        generic = [m.eval_packed(np.concatenate(c), rb.cu_of([len(s) for s in c])) for c in calls]
        m.set_option("attn", "mfma")
        assert [len(s) for s in calls[0]] == [600, 130] and _same(rows[0], generic[0])
        assert [len(s) for s in calls[1]] == [512, 130] and not _same(rows[1], generic[1])
    m.close()
