"""The kernels a model falls back to when the fused kernels refuse its shape, on their own: the generic mat-mul and attention
(gemm_naive_kernel, attention_naive_kernel), the pair-wise embedding and LayerNorm kernels (H % 8 != 0 or H > 1024 / 2048) and the row
kernels of misc_kernels.hip at every instantiation and edge -- through the op entries of libbert_test.so, every element against float64
on the same f16 or dequantised inputs within a bound derived from the kernel's roundings (layer_reference.py; test_value_bounds_host.py
checks the new ones without a GPU), with zeros and with quiet NaNs in every word the kernels do not own.  Then the two launches whose
grid.y a full host chunk overflows, the device API's max_len promise in the embedding kernels, and whole f16 / q4 models of odd
geometry.  Every test prints the worst fraction of its bound on a GENFRAC line; the docstrings record them (MI355X)."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

import layer_reference as ref
from conftest import cosine
from layer_reference import f8
from test_gpu_parity import MIN_COS, TIGHT_COS_PLAIN, WT, _q4_image_f16, _weight_bytes

pytestmark = pytest.mark.gpu

NAN16, NAN32 = 0x7E00, 0x7FC00000          # quiet NaN: data to the kernels, and it spreads to whatever reads it


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def _same_bits(a, b, what):
    neq = np.argwhere(_bits(a) != _bits(b))
    assert len(neq) == 0, (what, len(neq), neq[:8].tolist())


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _both_pads(call, what):
    """the call with zeros and with quiet NaNs in the rows behind the last token and in every output word: equal bits, no NaN"""
    got = call()
    with pybert.test_pad(NAN16, NAN32):
        _same_bits(call(), got, ("NaN pad", what))
    assert not np.isnan(got).any(), what
    return got


def _inside(got, want, bound, what):
    err = np.abs(f8(got) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(frac.max())
    print(f"GENFRAC {what}: worst fraction of the bound {worst:.3f}")
    assert worst <= 1, (what, worst, np.argwhere(frac > 1)[:5].tolist())
    return worst


def _ln_params(H):
    rng = np.random.default_rng(H)
    return (1 + rng.normal(0, 0.1, H)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# 1. LayerNorm widths
# ------------------------------------------------------------------------------------------------
# launch_layernorm: H % 8 == 0 and H <= 2048 -> layernorm_rows_kernel<1 | 2 | 4> (H <= 512 | 1024 | 2048), else layernorm_kernel<NJ>
# with ceil(H / 128) <= 1 | 3 | 6 | 8 | 32: the first and last width of every variant, and one between
LN_WIDTHS = [8, 384, 512, 520, 768, 1024, 1032, 2048, 2, 100, 126, 130, 380, 390, 764, 770, 1020, 2050, 4094]


@pytest.mark.parametrize("H", LN_WIDTHS)
def test_layernorm_widths(H):
    """launch_layernorm in place on f16 rows of layer_reference.layernorm_rows' classes (mean / std 0 .. 64 and an outlier; every
    class is in the domain of two-pass statistics): 33 rows, and 1, 3, 4 and 5 of them -- four rows a workgroup, ragged last groups --
    whose bits are those of the 33-row call.  The two-pass bound, no input term (the f16 rows are exact).
    Measured: worst fraction of the bound 0.49 (H = 8; the rounding to f16 is half the ulp allowed for it)."""
    _, rows, _ = ref.layernorm_rows(33, H, 9000 + H)
    x = rows.astype(np.float16)
    g, b = _ln_params(H)
    got = _both_pads(lambda: pybert.test_layernorm(x, g, b), H)
    want = ref.layernorm(f8(x), f8(g), f8(b))
    _inside(got, want, ref.layernorm_bound(f8(x), g, want), f"layernorm H {H}")
    for T in (1, 3, 4, 5):
        _same_bits(_both_pads(lambda: pybert.test_layernorm(x[:T], g, b), (H, T)), got[:T], (H, T))


# ------------------------------------------------------------------------------------------------
# 2. embedding + LayerNorm
# ------------------------------------------------------------------------------------------------
def _embed_form(ftype, H, lens, max_len):
    """launch_embed_ln's rule, restated: "grid" = the (4-token group, sentence) grid, "search" = one group per 4 tokens of the batch
    and a bisection of cu_seqlens, "pair" = embed_ln_kernel<NJ>"""
    n, T = len(lens), sum(lens)
    if not ((H % 8 == 0 if ftype in ("f32", "f16") else H % 32 == 0) and H <= 1024 and max_len > 0):
        return "pair"
    return "search" if n > 65535 or 2 * ((max_len + 3) // 4) * n > 3 * ((T + 3) // 4) else "grid"


def _embed_tables(ftype, H, n_vocab, n_pos, seed=0):
    """(file bytes, dequantised float64) of word, type and position tables; position rows are distinguishable, type row 1 is far off"""
    rng = np.random.default_rng(7 * H + n_vocab + seed)
    tabs = [rng.normal(0, 1, (n, H)).astype(np.float32) for n in (n_vocab, 2, n_pos)]
    tabs[1][1] += 100.0                                # (row 1 is not used: bert.cpp:800 adds type[0])
    tabs[2] += np.linspace(-2, 2, n_pos)[:, None].astype(np.float32)
    enc = [_weight_bytes(t, ftype) for t in tabs]
    return [e[0] for e in enc], [f8(e[1]).reshape(-1, H) for e in enc]


def _embed_check(ftype, H, lens, toks, byts, deq, g, b, got, what):
    word, typ, pos = deq
    p = np.concatenate([np.arange(n) for n in lens])
    inner = typ[0][None, :] + word[np.clip(toks, 0, len(word) - 1)]
    rows = pos[p] + inner
    want = ref.layernorm(rows, f8(g), f8(b))
    bound = ref.layernorm_bound(rows, g, want) + ref.layernorm_input_term(rows, g, ref.U32 * (np.abs(inner) + np.abs(rows)))
    return _inside(got, want, bound, what)


EMBED_LENS = [("grid", [33]), ("grid", [64, 64, 61]), ("search", [64, 1, 2, 3, 4, 5])]
EMBED_CASES = [(t, H) for t in ("f32", "f16", "q4_0", "q4_1") for H in (32, 384, 512, 544, 1024, 1056)] + \
              [(t, H) for t in ("f32", "f16") for H in (2, 100, 130, 390, 770)]


@pytest.mark.parametrize("ftype,H", EMBED_CASES)
def test_embed_ln(ftype, H):
    """word[id] + type[0] + pos[p] -> LayerNorm, tables of every file type: embed_ln_rows_kernel<TT, 1 | 2, SEARCH> in both grid
    forms (which one a batch takes is asserted from launch_embed_ln's rule, restated above), embed_ln_kernel<1 | 3 | 6 | 8> at
    H % 8 != 0 and <32> at H = 1056 (through table_elem for the q4 tables).  Ids -1 and n_vocab take the rows of 0 and n_vocab - 1.
    Against float64 on the dequantised tables: the two-pass LayerNorm bound plus what the two f32 additions in front can cost.
    Measured: worst fraction of the bound 0.50 (H = 32; 0.43 at H = 1056)."""
    n_vocab, n_pos = 50, 64
    byts, deq = _embed_tables(ftype, H, n_vocab, n_pos)
    g, b = _ln_params(H)
    for form, lens in EMBED_LENS:
        expect = "pair" if H % 8 != 0 or H > 1024 else form
        assert _embed_form(ftype, H, lens, max(lens)) == expect, (expect, lens)
        T = sum(lens)
        toks = np.random.default_rng(T + H).integers(0, n_vocab, size=T).astype(np.int32)
        toks[0], toks[-1], toks[T // 2], toks[T // 3] = -1, n_vocab, n_vocab - 1, 0
        got = _both_pads(lambda: pybert.test_embed_ln(WT[ftype], *byts, H, g, b, toks, _cu(lens)), (ftype, H, lens))
        _embed_check(ftype, H, lens, toks, byts, deq, g, b, got, f"embed {ftype} H {H} {expect} {lens}")
        clamped = np.clip(toks, 0, n_vocab - 1)
        _same_bits(pybert.test_embed_ln(WT[ftype], *byts, H, g, b, clamped, _cu(lens)), got, "ids -1 and n_vocab are ids 0 and n_vocab - 1")


def test_embed_ln_search_form_past_65535_sentences():
    """65537 one-token sentences at H = 8: more sentences than a grid dimension holds, so the SEARCH form whatever the lengths say
    (17 steps of bisection).  Measured: worst fraction of the bound 0.50."""
    n, H, n_vocab = 65537, 8, 50
    lens = [1] * n
    assert _embed_form("f16", H, lens, 1) == "search"
    byts, deq = _embed_tables("f16", H, n_vocab, 4)
    g, b = _ln_params(H)
    toks = (np.arange(n) * 7 % n_vocab).astype(np.int32)
    got = _both_pads(lambda: pybert.test_embed_ln(WT["f16"], *byts, H, g, b, toks, _cu(lens)), "65537 sentences")
    _embed_check("f16", H, lens, toks, byts, deq, g, b, got, "embed f16 H 8 search 65537 sentences")


@pytest.mark.parametrize("nan_from", ["40", "max_len"])
@pytest.mark.parametrize("max_len", [40, 38])
@pytest.mark.parametrize("form,H,extra", [("grid", 64, []), ("search", 64, [1]), ("pair", 100, [])])
def test_embed_ln_under_a_broken_max_len(form, H, extra, max_len, nan_from):
    """The device API's promise broken in the embedding: a position table of 80 rows whose rows from 40 on (and, second case, from
    max_len on: the grid form's positions stop at round_up(max_len, 4) - 1) are NaN, a sentence of 50 tokens under max_len = 40
    and 38.  Every written row of the offender is finite -- no row at or behind max_len was read -- and the other sentences have
    the bits of the same call with the offender cut to 40 tokens.  (The SEARCH form takes one more sentence, of one token: the four
    lengths alone choose the grid.)  Before the kernels clamped the position row 9 of the 12 cases failed -- every one of the SEARCH
    form and the pair kernel, whose position has no bound, and the grid form at max_len = 38 with NaN rows from 38 on; every row
    read lies inside the 80-row table either way."""
    lens = [20, 50, 33, 7] + extra
    assert _embed_form("f16", H, lens, max_len) == form
    n_vocab, n_pos = 50, 80
    byts, _ = _embed_tables("f16", H, n_vocab, n_pos, seed=1)
    pos = byts[2].view(np.uint16).reshape(n_pos, H).copy()
    pos[(40 if nan_from == "40" else max_len):] = NAN16
    byts[2] = pos.view(np.uint8).reshape(-1)
    g, b = _ln_params(H)
    cu = _cu(lens)
    toks = np.random.default_rng(H + max_len).integers(0, n_vocab, size=int(cu[-1])).astype(np.int32)
    got = pybert.test_embed_ln(WT["f16"], *byts, H, g, b, toks, cu, max_len)
    assert np.isfinite(got[cu[1]:cu[2]]).all(), ("a position row at or behind max_len was read", np.argwhere(~np.isfinite(got[cu[1]:cu[2]]))[:4].tolist())
    cut = [20, 40, 33, 7] + extra
    keep = np.r_[0:20, 20 + 40:sum(cut)]
    honest = pybert.test_embed_ln(WT["f16"], *byts, H, g, b, np.delete(toks, np.r_[60:70]), _cu(cut), max_len)
    _same_bits(got[np.r_[0:20, 70:int(cu[-1])]], honest[keep], "the other sentences")
    assert np.isfinite(honest[keep]).all()


# ------------------------------------------------------------------------------------------------
# 3. the generic mat-mul
# ------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (3, 7, 5), (5, 100, 100), (33, 136, 64), (4, 64, 33), (130, 65, 130), (257, 300, 20)]


def _stored(W, ftype):
    """(file bytes, the f16 image the generic kernel reads: GemmWeight::naive16) of W in the file type"""
    if ftype in ("f32", "f16"):
        return _weight_bytes(W, ftype)[0], W.astype(np.float16)
    q = gf.quantize_q4_0(W) if ftype == "q4_0" else gf.quantize_q4_1(W)
    return q.reshape(-1), _q4_image_f16(q, WT[ftype], W.shape)


# (q4 blocks hold 32 weights of a row: those file types where K % 32 == 0)
@pytest.mark.parametrize("M,N,K,ftype", [(*shp, t) for shp in GEMM_SHAPES for t in ("f32", "f16", "q4_0", "q4_1") if t[0] == "f" or shp[2] % 32 == 0])
def test_generic_gemm_shapes(M, N, K, ftype):
    """gemm_naive_kernel where no MFMA kernel goes: K and N multiples of nothing, one element, N behind the 64-lane feature block
    (n >= N), M behind the 4-row group (t >= M), all three epilogues, every file type whose blocks the row length allows.  Bound: an
    ascending f32 chain of K exact products, the bias, the epilogue, one f16 rounding (layer_reference.generic_gemm_bound).
    Measured: worst fraction of the bound 0.50 (bias, residual: the rounding to f16), 0.18 (GELU)."""
    A, W, bias, resid = ref.generic_gemm_inputs(M, N, K)
    wb, W16 = _stored(W + (0.03 if ftype == "q4_1" else 0), ftype)
    for epi in (0, 1, 2):
        r = resid if epi == 2 else None
        got = _both_pads(lambda: pybert.test_gemm(A, wb, WT[ftype], N, bias, r, epi, 1), (M, N, K, ftype, epi))
        bound, want = ref.generic_gemm_bound(A, W16, bias, r, epi)
        _inside(got, want, bound, f"gemm_naive {ftype} epi {epi} M {M} N {N} K {K}")


def test_generic_gemm_rows_do_not_depend_on_the_rows_behind_them():
    """Rows 0 .. M - 1 of a call at M have the bits of the same rows of the call at 257 (guards `t >= M` and the row index)."""
    A, W, bias, resid = ref.generic_gemm_inputs(257, 300, 20)
    wb = W.astype(np.float16).view(np.uint8).reshape(-1)
    for epi in (0, 1, 2):
        full = pybert.test_gemm(A, wb, 1, 300, bias, resid if epi == 2 else None, epi, 1)
        for M in (1, 3, 4, 5, 33, 130, 256):
            _same_bits(pybert.test_gemm(A[:M], wb, 1, 300, bias, resid[:M] if epi == 2 else None, epi, 1), full[:M], (epi, M))


def test_generic_gemm_at_a_full_chunk_of_tokens():
    """M = 262144, a host chunk's token count (options.h chunk_tokens): 65536 groups of 4 rows, one more than a grid dimension is
    assumed to hold (kernels.h GRID_YZ_MAX), so launch_gemm_naive makes two launches.  N = K = 8, bias epilogue, every element
    against float64; rows 0 .. 256 have the bits of the call at M = 257.  Measured: worst fraction of the bound 0.50."""
    M, N, K = 262144, 8, 8
    rng = np.random.default_rng(M)
    A = rng.normal(0, 1, (M, K)).astype(np.float16)
    W16 = (rng.normal(0, 1, (N, K)) / np.sqrt(K) * (1 + np.arange(K) / K)).astype(np.float16)
    bias = rng.normal(0, 0.5, N).astype(np.float32)
    wb = W16.view(np.uint8).reshape(-1)
    got = pybert.test_gemm(A, wb, 1, N, bias, None, 0, 1)
    bound, want = ref.generic_gemm_bound(A, W16, bias, None, 0)
    _inside(got, want, bound, "gemm_naive M 262144")
    _same_bits(pybert.test_gemm(A[:257], wb, 1, N, bias, None, 0, 1), got[:257], "rows of the M = 257 call")


# ------------------------------------------------------------------------------------------------
# 4. the generic attention
# ------------------------------------------------------------------------------------------------
ATT_LENS = (1, 2, 3, 4, 5, 63, 64, 65, 130)


@pytest.mark.parametrize("n_head,d_head", [(3, 2), (5, 20), (2, 33), (2, 64), (1, 96)])
def test_generic_attention_shapes(n_head, d_head):
    """attention_naive_kernel at d_head below, between and above the MFMA kernel's 32 and 64 (96: the output loop takes two
    strides of 64 lanes), sentences around the 64-key stride and the 4-query block (max_len = 130 is not a multiple of 4: the last
    block's waves have q >= n, a wave's stripe of scores is gridDim.x * 4 = 132 floats).  Every element inside the two-pass bound
    (layer_reference.generic_attention_bound), and every sentence alone gives the bits it has in the batch.
    Measured: worst fraction of the bound 0.49 (the rounding to f16)."""
    qkv = ref.generic_attention_inputs(ATT_LENS, n_head, d_head)
    cu = _cu(ATT_LENS)
    got = _both_pads(lambda: pybert.test_attention(qkv, cu, n_head, d_head, 1), (n_head, d_head))
    want, bound = ref.generic_attention_packed(qkv, ATT_LENS, n_head, d_head)
    _inside(got, want, bound, f"attention_naive heads {n_head} d {d_head}")
    for b, n in enumerate(ATT_LENS):
        rows = slice(cu[b], cu[b + 1])
        _same_bits(pybert.test_attention(qkv[rows], _cu([n]), n_head, d_head, 1), got[rows], ("alone", n))


def test_generic_attention_is_the_fallback_at_514_tokens():
    """A sentence of 514 tokens at d_head 64 (an mpnet-dims file: n_max_tokens 514): the keys pad to 640 and K plus V^T no longer fit
    a workgroup's LDS, launch_attention_mfma declines (-2) and the engine runs this kernel.
    Measured: worst fraction of the bound 0.38."""
    lens, n_head, d_head = (514,), 2, 64
    qkv = ref.generic_attention_inputs(lens, n_head, d_head)
    with pytest.raises(RuntimeError, match="failed: -2$"):
        pybert.test_attention(qkv, _cu(lens), n_head, d_head, 0)
    got = _both_pads(lambda: pybert.test_attention(qkv, _cu(lens), n_head, d_head, 1), "514")
    want, bound = ref.generic_attention_packed(qkv, lens, n_head, d_head)
    _inside(got, want, bound, "attention_naive 514 tokens d 64")


@pytest.mark.parametrize("n", [1, 17, 129])
def test_generic_attention_hard_softmax_cases(n, d=20):
    """layer_reference.SOFTMAX_CASES through this kernel: identical keys, one key 40 ahead, maxima 180 apart, scores of +-300 (whose
    exponentials v_exp_f32 flushes to zero), |V| up to 2^14 and in the subnormals.
    Measured: worst fraction of the bound 0.50 (subnormal-v); the ahead-* cases return one row of V exactly."""
    for case in ref.SOFTMAX_CASES:
        q, k, v = ref.softmax_case(case, n, d)
        qkv = np.concatenate([q, k, v], axis=1)
        got = _both_pads(lambda: pybert.test_attention(qkv, _cu([n]), 1, d, 1), case)
        bound, want = ref.generic_attention_bound(q, k, v)
        _inside(got, want, bound, f"attention_naive softmax {case} n {n} d {d}")


def test_generic_attention_past_65535_sentences():
    """65537 sentences of one token (a vocabulary list embedded word by word is three tokens a sentence: a host chunk holds up to
    87381 of those), 1 head of 8: more than a grid dimension is assumed to hold, so launch_attention_naive makes two launches, the
    second from cu_seqlens + 65535.  One key: the softmax is 1 and every output row is its V row, bit for bit."""
    n, d = 65537, 8
    qkv = np.random.default_rng(n).normal(0, 1, (n, 3 * d)).astype(np.float16)
    got = pybert.test_attention(qkv, _cu([1] * n), 1, d, 1)
    _same_bits(got, qkv[:, 2 * d:], "every row is its V row")


# ------------------------------------------------------------------------------------------------
# 5. whole models of odd geometry
# ------------------------------------------------------------------------------------------------
ODD_F16 = "h100-d20-i136-l2"
MIXED = {"f16": ("h128-d32-i136-l2", gf.BertHParams(300, 64, 128, 136, 4, 2)), "q4_0": ("h128-d32-i160-l2", gf.BertHParams(300, 64, 128, 160, 4, 2))}
ODD_HIDDEN_TOL = [3.4e-3, 7.9e-3, 1.02e-2]            # (per layer: twice what test_f16_model_of_odd_geometry measured)


def test_f16_model_of_odd_geometry(make_model):
    """H = 100, 5 heads of 20, I = 136, 70 positions, 2 layers, f16: no mat-mul has K % 64 == 0, so every one is the generic kernel's
    (the profile shows family:gemm_naive only), the attention is the generic one, the embedding and both LayerNorms the pair kernels.
    Embeddings against the oracle's plain mode (f32 arithmetic on the file's f16 weights): cosine at least TIGHT_COS_PLAIN; hidden
    states through eval_hidden within ODD_HIDDEN_TOL, twice the worst max-abs measured over the four sentences against the oracle on
    this model (1.68e-3 after the embedding, 3.90e-3 and 5.07e-3 after the layers: f16 activations against f32 ones); a sentence
    alone has the bits it has in the batch.  Measured: worst cosine 1 - 4.4e-7."""
    gf.MODEL_DIMS.setdefault(ODD_F16, gf.BertHParams(300, 70, 100, 136, 5, 2))
    path, hp = make_model(ODD_F16, "f16", 3)
    m = pybert.BertModel(path)
    o = orc.Oracle(path)
    rng = np.random.default_rng(21)
    sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in (1, 2, 33, 70)]
    m.profile(True)
    got = m.eval_batch(sents)
    rep = m.profile_report(families=True)
    m.profile(False)
    fam = {k: v["launches"] for k, v in rep.items() if k.startswith("family:")}
    assert list(fam) == ["family:gemm_naive"] and fam["family:gemm_naive"] == 4 * hp.n_layer, rep
    worst = min(cosine(g, o.eval(s, orc.MODE_PLAIN)) for s, g in zip(sents, got))
    print(f"GENFRAC odd f16 model: worst cosine against the plain oracle 1 - {1 - worst:.3e}")
    assert worst >= TIGHT_COS_PLAIN, worst
    assert np.array_equal(np.stack([m.eval(s) for s in sents]), got)
    for s in sents:
        emb, hid = m.eval_hidden(s)
        want_emb, want_hid = o.eval(s, orc.MODE_PLAIN, want_hidden=True)
        for layer in range(hp.n_layer + 1):
            err = float(np.abs(hid[layer] - want_hid[layer]).max())
            print(f"GENFRAC odd f16 model: hidden states n {len(s)} layer {layer} max-abs {err:.3e} of {ODD_HIDDEN_TOL[layer]:.3e}")
            assert err < ODD_HIDDEN_TOL[layer], (len(s), layer, err)
        assert cosine(emb, want_emb) >= TIGHT_COS_PLAIN
    m.close()


@pytest.mark.parametrize("ftype", ["f16", "q4_0"])
def test_model_that_mixes_kernel_families_in_a_layer(make_model, ftype):
    """H = 128, 4 heads of 32, I = 136: Q | K | V (the window kernel) and the output projection run on the matrix cores, the
    up-projection on gemm_mfma_kernel at N = 136 -- a partial second feature tile of 8 -- and the down-projection, K = 136, on the
    generic kernel: both families in the profile, one generic launch a layer.  A q4 file cannot have I = 136 (a row is whole blocks
    of 32; the loader refuses it as the reference does), so the q4_0 model has I = 160: N = 160 is again no multiple of 64 and
    K = 160 none of 64.  Thresholds of test_eval_matches_oracle_small.  Measured: worst cosine against the ggml-mode oracle
    1 - 6.4e-7 (f16)."""
    dims, hparams = MIXED[ftype]
    gf.MODEL_DIMS.setdefault(dims, hparams)
    path, hp = make_model(dims, ftype, 4)
    m = pybert.BertModel(path)
    o = orc.Oracle(path)
    rng = np.random.default_rng(5)
    sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in (1, 2, 3, 17, 31, 32, 33, 48, 64)]
    m.profile(True)
    got = m.eval_batch(sents)
    rep = m.profile_report(families=True)
    m.profile(False)
    fam = {k: v["launches"] for k, v in rep.items() if k.startswith("family:")}
    # (a q4 file's matrices are expanded to f16 images at load unless BERT_HIP_Q4=fused: gemm_mfma_f16 either way here)
    assert sorted(fam) == ["family:gemm_mfma_f16", "family:gemm_naive"] and fam["family:gemm_naive"] == hp.n_layer, rep
    assert fam["family:gemm_mfma_f16"] in (2 * hp.n_layer, 3 * hp.n_layer), rep
    coss = []
    for s, g in zip(sents, got):
        want, plain = o.eval(s, orc.MODE_GGML), o.eval(s, orc.MODE_PLAIN)
        assert abs(np.linalg.norm(g) - 1) < 1e-3
        coss.append(cosine(g, want))
        assert coss[-1] >= MIN_COS[ftype], (ftype, len(s), coss[-1])
        if ftype == "q4_0":
            assert cosine(g, plain) >= min(cosine(want, plain), 1 - 1e-4) - 1e-4
        else:
            assert cosine(g, plain) >= 1 - 1e-4
    print(f"GENFRAC mixed {ftype} model: worst cosine against the ggml-mode oracle 1 - {1 - min(coss):.3e}")
    assert np.array_equal(np.stack([m.eval(s) for s in sents]), got)
    m.close()
