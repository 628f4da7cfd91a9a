"""The f32 route's five kernels (f32_route.hip) on their own, through the bert_hip_test_f32_* entries of libbert_test.so: every
element against a float64 restatement within a bound derived from the kernel's roundings (f32_reference.py, which
test_f32_bounds_host.py checks without a GPU), at the shapes the model files of the other tests never reach -- K, N, H, d_head that are
multiples of nothing, partial tiles, one-token sentences, empty ones -- and with quiet NaNs in every word the kernels do not own.  Then
a whole model of odd geometry, the device API's max_len promise on the route, and the host's refusal of a max_len whose scores do not
fit in LDS."""
import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

import f32_reference as f32
import layer_reference as ref
from f32_reference import f4, f8

pytestmark = pytest.mark.gpu

NAN16, NAN32 = 0x7E00, 0x7FC00000          # quiet NaN: data to the kernels, and it spreads to whatever reads it


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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
    print(f"F32FRAC {what}: worst fraction of the bound {worst:.3f}")
    assert worst <= 1, (what, worst, np.argwhere(frac > 1)[:5].tolist())
    return worst


# ------------------------------------------------------------------------------------------------
# mat-mul
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", f32.GEMM_SHAPES)
def test_gemm_shapes(M, N, K):
    """f32_gemm_kernel at every path of its staging (K % 4, the partial reduction tile K % 16, odd K: the upper half-wave adds zeros),
    of its feature tile (N % 64) and stores (N % 4, n + e < N) and of its token block (m >= M), under all three epilogues, with zeros
    and NaNs around.  Reported, not asserted: the share of elements whose bits equal ONE ascending f32 fma chain (f32_reference.fma_chain).
    Measured on the MI355X, worst fraction of the bound over the 40 shapes: bias 0.907, bias + GELU 0.368, bias + residual
    0.934 (all three at K = 1, where the bound is two roundings; 0.13 at K = 17 and less beyond); chain agreement 100 %: all 616 008
    elements of the bias and bias + residual calls, at every shape."""
    A, W, bias, resid = f32.gemm_inputs(M, N, K)
    for epi, r in ((f32.EPI_BIAS, None), (f32.EPI_GELU, None), (f32.EPI_RESID, resid)):
        got = _both_pads(lambda: pybert.test_f32_gemm(A, W, bias, r, epi), (M, N, K, epi))
        bound, want = f32.gemm_bound(A, W, bias, r, epi)
        _inside(got, want, bound, f"gemm epi {epi} M {M} N {N} K {K}")
        if epi != f32.EPI_GELU:
            same = _bits(got) == _bits(f32.fma_chain(A, W, bias, r))
            print(f"F32CHAIN epi {epi} M {M} N {N} K {K}: {same.sum()} of {same.size} elements have the bits of the ascending fma chain")


def test_gemm_rows_do_not_depend_on_the_rows_behind_them():
    """The prefix property test_gpu_padding_poison.py asserts for the f16 kernels: rows 0 .. M - 1 of a call at M have the bits of the
    same rows of a call at M' > M (a token's row is made of its own row of A only; guards `m >= M` and the staging's `am < M`)."""
    A, W, bias, resid = f32.gemm_inputs(129, 130, 100)
    for epi, r in ((f32.EPI_BIAS, None), (f32.EPI_GELU, None), (f32.EPI_RESID, resid)):
        full = pybert.test_f32_gemm(A, W, bias, r, epi)
        for M in (1, 33, 64, 65):
            _same_bits(pybert.test_f32_gemm(A[:M], W, bias, None if r is None else r[:M], epi), full[:M], (epi, M))


@pytest.mark.parametrize("bias", ["zero", "f32"])
def test_gelu_epilogue_over_the_sweep(bias):
    """The GELU epilogue alone: K = 1 and W = 1 make the pre-activation x + bias, x over layer_reference.gelu_sweep() (normal values
    only), against the bound that is absolute in the error of 1 + tanh.  The one term of it that is measured, not derived, is the
    device tanhf: worst 1.244 ulp over the sweep's 461 312 arguments on the MI355X, 2.49 allowed (f32_reference.TANHF_ULP).
    No NaN, nothing positive for a negative argument.  Measured: worst fraction of the bound 0.369."""
    x = ref.gelu_sweep()
    x = x[np.abs(f8(x)) >= 2.0 ** -14]
    A = f4(x)[:, None]
    W = np.ones((64, 1), np.float32)
    b = ref.gelu_biases(64)[bias]
    got = _both_pads(lambda: pybert.test_f32_gemm(A, W, b, None, f32.EPI_GELU), bias)
    bound, want = f32.gemm_bound(A, W, b, None, f32.EPI_GELU)
    _inside(got, want, bound, f"gelu sweep bias {bias}")
    pre = f8(A) + f8(b)[None, :]
    assert (f8(got)[pre < 0] <= 0).all() and (f8(got)[pre > 0] >= 0).all()


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
ATT_LENS = [(1, 2, 3, 4, 5, 63, 64, 65, 127, 129), (200, 7)]


@pytest.mark.parametrize("lens", ATT_LENS, ids=["ten", "200-7"])
@pytest.mark.parametrize("n_head,d_head", [(2, 32), (5, 20), (1, 65), (2, 96), (3, 7)])
def test_attention_shapes(n_head, d_head, lens):
    """f32_attention_kernel at d_head above 64 and a multiple of nothing, sentences around the 64-key stride and the 4-query block
    (the last block's waves have q >= n), max_len equal to the longest sentence and again longest + 3 (a wave's stripe of scores is
    a function of max_len, not of n): equal bits between the two, every element inside the bound, and every sentence alone gives the
    bits it has in the batch.  Measured: worst fraction of the bound 0.090 (3 heads of 7)."""
    qkv = f32.attention_inputs(lens, n_head, d_head)
    cu, longest = _cu(lens), max(lens)
    got = _both_pads(lambda: pybert.test_f32_attention(qkv, cu, n_head, d_head, longest), (lens, "max_len = longest"))
    _same_bits(_both_pads(lambda: pybert.test_f32_attention(qkv, cu, n_head, d_head, longest + 3), (lens, "longest + 3")), got,
               "max_len = longest + 3")
    want, bound = f32.attention_packed(qkv, lens, n_head, d_head, bound=True)
    _inside(got, want, bound, f"attention heads {n_head} d {d_head} lens {lens}")
    for b, n in enumerate(lens):
        rows = slice(cu[b], cu[b + 1])
        _same_bits(pybert.test_f32_attention(qkv[rows], _cu([n]), n_head, d_head, n), got[rows], ("alone", n))


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("n", [17, 129])
def test_attention_hard_softmax_cases(n, d):
    """layer_reference.SOFTMAX_CASES through this kernel (their f16 values are exact and normal in f32): identical keys, one key 40
    ahead, maxima 180 apart, scores of +-300, |V| up to 2^14.  Measured: worst fraction of the bound 0.067 (wide); the ahead-* cases
    return one row of V exactly (0.000)."""
    for case in ref.SOFTMAX_CASES:
        q, k, v = ref.softmax_case(case, n, d)
        qkv = f4(np.concatenate([q, k, v], axis=1))
        got = _both_pads(lambda: pybert.test_f32_attention(qkv, _cu([n]), 1, d, n), case)
        bound, want = f32.softmax_bound(q, k, v)
        _inside(got, want, bound, f"softmax {case} n {n} d {d}")


def test_attention_leaves_a_sentence_longer_than_max_len_alone():
    """The device API's promise broken at op level: a sentence of 12 tokens under max_len = 8 does not fit a wave's stripe of
    scores.  Its waves return before they touch LDS or write a row (the rows keep what the buffer held), the status word and the NaN
    row are the pooling kernel's; every other sentence keeps the bits it has under an honest max_len.  Guards the stripe bound
    `n > max_len`; no value-changing mutation reaches it."""
    lens, n_head, d_head = (5, 12, 3, 8), 2, 20
    qkv, cu = f32.attention_inputs(lens, n_head, d_head), _cu(lens)
    honest = pybert.test_f32_attention(qkv, cu, n_head, d_head, 12)
    keep = np.r_[0:5, 17:28]
    for pad32 in (0, NAN32):
        with pybert.test_pad(NAN16 if pad32 else 0, pad32):
            got = pybert.test_f32_attention(qkv, cu, n_head, d_head, 8)
        _same_bits(got[keep], honest[keep], ("neighbours", pad32))
        assert (_bits(got[5:17]) == pad32).all(), pad32


def test_attention_refuses_a_max_len_that_does_not_fit_in_lds():
    """64 ceil(max_len / 4) bytes of dynamic LDS a workgroup; above the device's limit (its properties' sharedMemPerBlock) the
    launcher refuses on the host and launches nothing: the entry's "not supported" code, -2.  Guards launch_f32_attention's check
    (before it, the runtime rejected the launch and the pass went on).  The MI355X gives a workgroup 163 840 bytes: max_len = 10240
    is the largest that runs (above 64 KiB the launcher opts the kernel in), 10241 the first refused."""
    lens, n_head, d_head = (3, 3), 2, 20
    qkv, cu = f32.attention_inputs(lens, n_head, d_head), _cu(lens)
    with pytest.raises(RuntimeError, match="failed: -2$"):
        pybert.test_f32_attention(qkv, cu, n_head, d_head, 1 << 22)
    with pytest.raises(RuntimeError, match="failed: -2$"):
        pybert.test_f32_attention(qkv, cu, n_head, d_head, 0)
    with pytest.raises(RuntimeError, match="failed: -2$"):
        pybert.test_f32_attention(qkv, cu, n_head, d_head, 10241)
    want = pybert.test_f32_attention(qkv, cu, n_head, d_head, 3)
    for max_len in (4096, 10240):
        _same_bits(pybert.test_f32_attention(qkv, cu, n_head, d_head, max_len), want, max_len)


# ------------------------------------------------------------------------------------------------
# LayerNorm, embedding
# ------------------------------------------------------------------------------------------------
LN_WIDTHS = [1, 7, 63, 64, 65, 100, 384]


@pytest.mark.parametrize("H", LN_WIDTHS)
def test_layernorm_widths(H):
    """f32_layernorm_row below one wave's 64 lanes (idle lanes enter the wave sums with zeros), at and around 64, on 23 rows (the last
    block of 4 tokens is partial) of layernorm_rows' classes: mean / std 0 .. 64 and an outlier, all in the domain of two-pass
    statistics.  Measured: worst fraction of the bound 0.091 (H = 7)."""
    v, g, b, _ = f32.layernorm_inputs(H, 23)
    got = _both_pads(lambda: pybert.test_f32_layernorm(v, g, b), H)
    want = ref.layernorm(f8(v), f8(g), f8(b))
    _inside(got, want, f32.layernorm_bound(v, g, want), f"layernorm H {H}")


def _embed_tables(H, n_vocab, n_pos):
    rng = np.random.default_rng(5 * H + n_vocab)
    word, type_, pos = (f4(rng.normal(0, 1, (n, H))) for n in (n_vocab, 2, n_pos))
    type_[1] += 100.0                                 # (row 1 is not used: bert.cpp:800 adds type[0])
    return word, type_, pos, f4(1 + rng.normal(0, 0.1, H)), f4(rng.normal(0, 0.1, H))


EMBED_LENS = {
    "one": [70], "two": [1, 69], "three": [1, 70, 1], "empty-neighbours": [1, 0, 3, 0, 0, 2, 1, 0],
    "thousand": [1] + [1 + (7 * i) % 3 for i in range(998)] + [1],
}


@pytest.mark.parametrize("H,batch", [(H, "three") for H in LN_WIDTHS] + [(65, b) for b in ("one", "two", "empty-neighbours", "thousand")] +
                         [(7, "thousand")])
def test_embed_ln(H, batch):
    """f32_embed_ln_kernel: ids 0 and n_vocab - 1, positions up to n_pos - 1, one-token sentences first and last, empty sentences
    beside them, 1, 2, 3 and 1000 sentences under the binary search.  Against float64 within the LayerNorm bound plus what the two
    f32 additions in front of it can cost.  Measured: worst fraction of the bound 0.094 (H = 7, 1000 sentences)."""
    n_vocab, n_pos = 50, 70
    word, type_, pos, g, b = _embed_tables(H, n_vocab, n_pos)
    lens = EMBED_LENS[batch]
    T = sum(lens)
    toks = np.random.default_rng(T).integers(0, n_vocab, size=T).astype(np.int32)
    toks[0], toks[-1], toks[T // 2] = 0, n_vocab - 1, n_vocab - 1
    got = _both_pads(lambda: pybert.test_f32_embed_ln(word, type_, pos, g, b, toks, _cu(lens), n_pos), (H, batch))
    rows, drows = f32.embed_rows(word, type_, pos, toks, lens)
    want = ref.layernorm(rows, f8(g), f8(b))
    _inside(got, want, f32.layernorm_bound(rows, g, want) + ref.layernorm_input_term(rows, g, drows), f"embed H {H} {batch}")
    # a smaller honest max_len changes nothing
    _same_bits(pybert.test_f32_embed_ln(word, type_, pos, g, b, toks, _cu(lens), max(lens)), got, "max_len = longest")


def test_embed_ln_under_a_broken_max_len():
    """A sentence of 9 tokens under max_len = 5: its tokens at places 0 .. 4, and every other sentence, have the bits of the honest
    call; what the rest of it holds does not matter (its embedding is the pooling kernel's NaN row) -- the kernel reads no position
    row at or behind max_len, which a run cannot show and the code does (`min(t - cu[lo], max_len - 1)`)."""
    word, type_, pos, g, b = _embed_tables(65, 50, 70)
    lens = [3, 9, 2]
    toks = np.arange(14, dtype=np.int32)
    honest = pybert.test_f32_embed_ln(word, type_, pos, g, b, toks, _cu(lens), 9)
    got = pybert.test_f32_embed_ln(word, type_, pos, g, b, toks, _cu(lens), 5)
    keep = np.r_[0:8, 12:14]
    _same_bits(got[keep], honest[keep], "places below max_len")


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 100, 256, 257, 384])
def test_pool_modes_and_guards(H):
    """f32_pool_normalize_kernel below and beside its 256 threads (waves that summed nothing still write a valid partial sum), in all
    four modes, with a sentence of max_len + 1 tokens and an empty one in the batch: NaN rows and status 1 for those two, every other
    row inside the bound, the CLS-raw row the stored f32 row exactly; without the two, status 0 and the same bits.
    Measured: worst fraction of the bound: mean raw 0.368, mean normalised 0.065, CLS normalised 0.250 (H = 1), CLS raw 0."""
    max_len = 9
    lens = [3, max_len + 1, 1, 0, max_len, 2]
    cu = _cu(lens)
    x = f4(np.random.default_rng(H).normal(0.1, 1, (int(cu[-1]), H)))
    good = [0, 2, 4, 5]
    for pooling in ("mean", "cls"):
        for normalize in (True, False):
            got, st = pybert.test_f32_pool(x, cu, max_len, pooling, normalize)
            with pybert.test_pad(NAN16, NAN32):
                got_nan, st_nan = pybert.test_f32_pool(x, cu, max_len, pooling, normalize)
            assert st == 1 and st_nan == 1
            assert np.isnan(got[[1, 3]]).all() and np.isnan(got_nan[[1, 3]]).all() and not np.isnan(got[good]).any()
            _same_bits(got_nan[good], got[good], ("NaN pad", pooling, normalize))
            for s in good:
                rows = x[cu[s]:cu[s + 1]]
                if (pooling, normalize) == ("cls", False):
                    _same_bits(got[s], rows[0], "cls raw")
                bound, want = f32.pool_bound(rows, pooling, normalize)
                _inside(got[s], want, bound, f"pool H {H} {pooling} normalize {normalize} n {len(rows)}")
            alone, st = pybert.test_f32_pool(np.concatenate([x[cu[s]:cu[s + 1]] for s in good]), _cu([lens[s] for s in good]), max_len,
                                             pooling, normalize)
            assert st == 0
            _same_bits(alone, got[good], ("without the offenders", pooling, normalize))


# ------------------------------------------------------------------------------------------------
# a whole model, the device API
# ------------------------------------------------------------------------------------------------
ODD = "h100-d20-i136-l2"


def test_f32_model_of_odd_geometry(make_model):
    """H = 100, 5 heads of 20, I = 136, 70 positions, 2 layers, f32: nothing a multiple of 16.  The profile shows the f32 mat-mul
    family only; embeddings and hidden states against the oracle's plain mode at the tolerances of
    test_f32_files_run_in_f32_arithmetic (2e-5 per component) and test_f32_route_hidden_states (2e-4 (1 + layer)).  The loader and
    the oracle take the geometry as it is; measured max-abs of the embeddings 1.5e-7."""
    gf.MODEL_DIMS.setdefault(ODD, gf.BertHParams(300, 70, 100, 136, 5, 2))
    path, hp = make_model(ODD, "f32", 3)
    m = pybert.BertModel(path)
    o = orc.Oracle(path)
    rng = np.random.default_rng(21)
    sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in (1, 2, 33, 70)]
    m.profile(True)
    got = m.eval_batch(sents)
    rep = m.profile_report(families=True)
    m.profile(False)
    assert rep.get("family:gemm_f32", {}).get("launches") == 4 * hp.n_layer and not any(k.startswith("family:gemm") and k != "family:gemm_f32" for k in rep), rep
    worst = max(float(np.abs(g - o.eval(s, orc.MODE_PLAIN)).max()) for s, g in zip(sents, got))
    print(f"F32FRAC odd model: embeddings max-abs {worst:.3e} of 2e-5")
    assert worst <= 2e-5, worst
    assert np.array_equal(np.stack([m.eval(s) for s in sents]), got)
    for s in (sents[2], sents[3]):
        emb, hid = m.eval_hidden(s)
        want_emb, want_hid = o.eval(s, orc.MODE_PLAIN, want_hidden=True)
        for layer in range(hp.n_layer + 1):
            assert np.abs(hid[layer] - want_hid[layer]).max() < 2e-4 * (1 + layer), (len(s), layer)
        assert np.abs(emb - want_emb).max() <= 2e-5


def test_device_api_guards_on_the_f32_route(make_model, capfd):
    """test_device_api_guards (test_multi_device.py) for an f32 file: a sentence of 50 tokens under a promise of 40 gets a NaN row and
    raises the status word once; every other sentence keeps the bits of bert_hip_eval_packed.  (Every length stays below the file's
    n_max_tokens of 64.)  Guards f32_attention_kernel's `n > max_len`: without it the offender's waves write their scores over their
    neighbours' stripes and past the workgroup's LDS."""
    from test_multi_device import _Hip
    hip = _Hip()
    path, hp = make_model("tiny", "f32", 0)
    m = pybert.BertModel(path)
    lens = [20, 50, 33, 7]
    cu = _cu(lens)
    T, H = int(cu[-1]), hp.n_embd
    toks = np.random.default_rng(0).integers(0, hp.n_vocab, size=T).astype(np.int32)
    m.profile(True)
    want = m.eval_packed(toks, cu)
    assert "family:gemm_f32" in m.profile_report(families=True)
    m.profile(False)
    d_t, d_cu = hip.upload(toks), hip.upload(cu)
    out = hip.upload(np.full((4, H), 7.0, np.float32))
    m.reserve(T, 4)
    m.eval_packed_device(d_t, d_cu, 4, T, 64, out, 0)
    assert m.check() == 0
    assert np.array_equal(hip.download(out, (4, H)), want)
    m.eval_packed_device(d_t, d_cu, 4, T, 40, out, 0)
    assert m.check() == 1 and m.check() == 0
    got = hip.download(out, (4, H))
    assert np.isnan(got[1]).all() and np.array_equal(got[[0, 2, 3]], want[[0, 2, 3]])
    assert "max_len" in capfd.readouterr().err
    m.eval_packed_device(d_t, d_cu, 4, T, 64, out, 0)
    assert m.check() == 0 and np.array_equal(hip.download(out, (4, H)), want)
