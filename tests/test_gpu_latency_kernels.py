"""The latency route's kernels (skinny.hip) on their own, through the op-level entries of libbert_test.so: bit for bit against the
batch route's kernels (which have float64 tests of their own in test_gpu_parity.py), every intermediate against float64, at the
widths that decide how the down-projection's pipeline starts and ends (I / 128 = 2, 3, 5, 8, 12, 20 batches of k-steps, four in
flight), at token counts around the 32-token block, and with NaN in the padding rows the kernels read.  Then whole models of the
widths no other test runs, and the hidden-state tap, through the route."""
import functools

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

import layer_reference as ref
from conftest import cosine
from test_gpu_parity import Q2_CASES, TIGHT_COS_GGML

pytestmark = pytest.mark.gpu

WIDTHS = [256, 384, 640, 1024, 1536, 2560]          # I / 128 = 2, 3 (fewer batches than slots), 5 (partial last round), 8, 12, 20 (all of LDS)
TOKENS = [1, 31, 32, 33, 128, 200]
# every width at a partial and at several token blocks, every token count at a partial-round and at an exact width, 768 tokens once per H
TAIL_CASES = sorted({(M, H, I) for H in (256, 384) for I in WIDTHS for M in (33, 200)} |
                    {(M, H, I) for H in (256, 384) for I in (640, 1536) for M in TOKENS} | {(768, 256, 640), (768, 384, 1536)})
NAN16, NAN32 = 0x7E00, 0x7FC00000                   # quiet NaN: ordinary data to the matrix cores, and it spreads to whatever reads it
PAD_TOKENS = (1, 33, 200)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(a, b, what):
    neq = np.argwhere(_bits(a) != _bits(b))
    assert len(neq) == 0, (what, len(neq), neq[:8].tolist())


@functools.lru_cache(maxsize=2)
def _tail_inputs(M, H, I):
    """test_layer_tail_kernel's distributions, k asymmetric (a permuted k-tile cannot pass), parameters as the f32 the device gets."""
    rng = np.random.default_rng(1000003 * M + 1009 * H + I)
    ctx = rng.normal(0, 1, (M, H)).astype(np.float16)
    x = rng.normal(0, 1, (M, H)).astype(np.float16)
    Ws = []
    for n, k in ((H, H), (I, H), (H, I)):
        w = rng.normal(0, 1, (n, k)) / np.sqrt(k)
        w[:, : k // 2] *= 1.3
        Ws.append(w.astype(np.float16))
    f4 = lambda a: a.astype(np.float32)
    bo, b2 = f4(rng.normal(0, 0.2, H)), f4(rng.normal(0, 0.2, H))
    b1 = f4(rng.normal(0, 0.5, I))
    g1, g2 = f4(1 + rng.normal(0, 0.1, H)), f4(1 + rng.normal(0, 0.1, H))
    be1, be2 = f4(rng.normal(0, 0.1, H)), f4(rng.normal(0, 0.1, H))
    return dict(ctx=ctx, x=x, Wo=Ws[0], W1=Ws[1], W2=Ws[2], bo=bo, g1=g1, be1=be1, b1=b1, b2=b2, g2=g2, be2=be2)


def _tail_args(d, I):
    return (d["ctx"], d["x"], d["Wo"].view(np.uint8), d["W1"].view(np.uint8), d["W2"].view(np.uint8), 1, I,
            d["bo"], d["g1"], d["be1"], d["b1"], d["b2"], d["g2"], d["be2"])


def _qkv_weights(H):
    """test_qkv_attention2_kernel's distributions"""
    rng = np.random.default_rng(77 + H)
    W = rng.normal(0, 1, (3 * H, H)) / np.sqrt(H)
    W[:H] *= 1.7
    W[:, : H // 2] *= 1.3
    return W.astype(np.float16), rng.normal(0, 0.3, 3 * H).astype(np.float32)


def _natural_order(ff):
    """SK_UP stores the runs of 4 features of every group of 16 at [0-3, 8-11, 4-7, 12-15]: the two middle runs change places."""
    M, I = ff.shape
    return np.ascontiguousarray(ff.reshape(M, I // 16, 4, 4)[:, :, [0, 2, 1, 3], :]).reshape(M, I)


@pytest.mark.parametrize("M,H,I", TAIL_CASES)
def test_skinny_tail_has_the_one_launch_tail_s_bits_and_float64_parts(M, H, I):
    """PROJ, UP (LayerNorm 1 fused), DOWN, LayerNorm 2 as Engine::forward_latency launches them: the output has the bits of
    layer_tail.hip's; every intermediate sits within a derived bound of float64 arithmetic on what the kernel read.
    Worst measured on the MI355X over the 42 cases: v_proj err / S 1.72e-7 and v_down err / S 2.86e-7 (0.3 % of their bounds);
    y 0.80 of its bound (a value that beta all but cancels; 0.49 - 0.67 elsewhere: the rounding to f16); ff 0.39 of its bound;
    the whole tail max 2.6e-3, mean 3.3e-4."""
    d = _tail_inputs(M, H, I)
    args = _tail_args(d, I)
    got, p = pybert.test_skinny_tail(*args, pad=0, parts=True)
    _same_bits(got, pybert.test_layer_tail(*args, 1), "layer_tail.hip")

    # the whole tail against the float64 restatement test_layer_tail_kernel uses, and that test's bounds
    want = ref.layer_tail(d["ctx"], d["x"], d["Wo"], d["W1"], d["W2"], d["bo"], d["g1"], d["be1"], d["b1"], d["b2"], d["g2"], d["be2"])
    err = np.abs(ref.f8(got) - want)
    print(f"tail M={M} H={H} I={I}: max {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() < 2.5e-2 and err.mean() < 2e-3, (float(err.max()), float(err.mean()))

    # out-projection: ctx Wo^T + bo + x, f32
    bound, S = ref.matmul_bound(d["ctx"], d["Wo"], d["bo"], d["x"])
    err = np.abs(ref.f8(p["v_proj"]) - (ref.f8(d["ctx"]) @ ref.f8(d["Wo"]).T + ref.f8(d["bo"]) + ref.f8(d["x"])))
    print(f"  v_proj err/S {(err / S).max():.3e} of {4 * (H + 4) * 2.0 ** -24:.3e}")
    assert (err <= bound).all(), ("v_proj", float((err / S).max()), np.argwhere(err > bound)[:5].tolist())

    # LayerNorm 1 of the rows the kernel read back: one f16 ulp of the value + 1e-5 |value| for the f32 statistics
    want = ref.layernorm(ref.f8(p["v_proj"]), ref.f8(d["g1"]), ref.f8(d["be1"]))
    err = np.abs(ref.f8(p["y"]) - want)
    bound = ref.f8(np.spacing(np.abs(want).astype(np.float16))) + 1e-5 * np.abs(want)
    print(f"  y err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), ("y", float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())

    # up-projection + GELU on the y the kernel wrote, un-permuted: the bound test_gemm_kernel holds a GEMM + GELU epilogue to
    ff = _natural_order(p["ff"])
    want = ref.gelu(ref.f8(p["y"]) @ ref.f8(d["W1"]).T + ref.f8(d["b1"]))
    err = np.abs(ref.f8(ff) - want)
    bound = 2e-3 * np.abs(want) + 4e-3
    print(f"  ff err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), ("ff", float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())

    # down-projection: ff W2^T + b2 + y, f32, on the ff and y the kernels wrote
    want = ref.f8(ff) @ ref.f8(d["W2"]).T + ref.f8(d["b2"]) + ref.f8(p["y"])
    bound, S = ref.matmul_bound(ff, d["W2"], d["b2"], p["y"])
    err = np.abs(ref.f8(p["v_down"]) - want)
    print(f"  v_down err/S {(err / S).max():.3e} of {4 * (I + 4) * 2.0 ** -24:.3e}")
    assert (err <= bound).all(), ("v_down", float((err / S).max()), np.argwhere(err > bound)[:5].tolist())

    # "the next QKV kernel writes the same bits again" (Engine::forward_latency): the LayerNorm-fused projection of the next layer,
    # given this tail's f32 rows and LayerNorm 2, writes this tail's output as its ln_out, and projects exactly those rows
    Wq, bq = _qkv_weights(H)
    qkv, ln_out = pybert.test_skinny_qkv(Wq.view(np.uint8), 1, bq, V=p["v_down"], gamma=d["g2"], beta=d["be2"])
    _same_bits(ln_out, got, "ln_out of the next layer's projection")
    _same_bits(qkv, pybert.test_skinny_qkv(Wq.view(np.uint8), 1, bq, x=ln_out), "fused projection against the plain one on its ln_out")

    # rows below M do not depend on the rows at and above M the kernels read
    if M in PAD_TOKENS:
        got_nan, p_nan = pybert.test_skinny_tail(*args, pad=NAN16, parts=True)
        _same_bits(got_nan, got, "NaN padding: out")
        for k in p:
            _same_bits(p_nan[k], p[k], "NaN padding: " + k)
        assert not np.isnan(got).any()


@pytest.mark.parametrize("H", [256, 384])
@pytest.mark.parametrize("M", TOKENS + [768])
def test_skinny_qkv_projection(M, H):
    """The plain form (x as f16 rows) against the tiled GEMM kernel, whose k sequence qkv_attention2 and this kernel share; the
    LayerNorm-fused form against the plain form on the rows it wrote, and those rows against a float64 LayerNorm."""
    rng = np.random.default_rng(31 * M + H)
    x = rng.normal(0, 1, (M, H)).astype(np.float16)
    V = rng.normal(0.1, 1.5, (M, H)).astype(np.float32)
    g, be = (1 + rng.normal(0, 0.1, H)).astype(np.float32), rng.normal(0, 0.1, H).astype(np.float32)
    W, bias = _qkv_weights(H)
    wb = W.view(np.uint8)
    plain = pybert.test_skinny_qkv(wb, 1, bias, x=x)
    _same_bits(plain, pybert.test_gemm(x, wb, 1, 3 * H, bias, None, 0, 0), "gemm.hip")
    qkv, ln_out = pybert.test_skinny_qkv(wb, 1, bias, V=V, gamma=g, beta=be)
    _same_bits(qkv, pybert.test_skinny_qkv(wb, 1, bias, x=ln_out), "fused projection against the plain one on its ln_out")
    want = ref.layernorm(ref.f8(V), ref.f8(g), ref.f8(be))
    err = np.abs(ref.f8(ln_out) - want)
    bound = ref.layernorm_bound(V, g, want)
    print(f"qkv M={M} H={H}: ln_out err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), ("ln_out", float((err / bound).max()), np.argwhere(err > bound)[:5].tolist())
    if M in PAD_TOKENS:
        _same_bits(pybert.test_skinny_qkv(wb, 1, bias, x=x, pad=NAN16), plain, "NaN padding: plain")
        qkv_nan, ln_nan = pybert.test_skinny_qkv(wb, 1, bias, V=V, gamma=g, beta=be, pad=NAN32)
        _same_bits(qkv_nan, qkv, "NaN padding: fused qkv")
        _same_bits(ln_nan, ln_out, "NaN padding: ln_out")
        assert not np.isnan(plain).any() and not np.isnan(qkv).any()


def _at_most(lens, n_tokens):
    return [n for n, total in zip(lens, np.cumsum(lens)) if total <= n_tokens]


@pytest.mark.parametrize("n_head", [8, 12])
@pytest.mark.parametrize("lens", [Q2_CASES[1], _at_most(Q2_CASES[3], 768), Q2_CASES[5], [128]], ids=["edges", "short", "mixed", "one-full"])
def test_skinny_qkv_then_attention_is_the_window_kernel(n_head, lens):
    """The first half of a latency-route layer (feature-split projection, then attention.hip) gives the bits of qkv_attention2
    and of the GEMM kernel + attention.hip."""
    assert sum(lens) <= 768
    d_head, H = 32, 32 * n_head
    rng = np.random.default_rng(sum(lens) + n_head)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = rng.normal(0, 1, (int(cu[-1]), H)).astype(np.float16)
    W, bias = _qkv_weights(H)
    got, windows, split = (pybert.test_qkv_attention(x, cu, n_head, d_head, W.view(np.uint8), 1, bias, mode) for mode in (5, 2, 0))
    _same_bits(got, windows, "qkv_attention2")
    _same_bits(got, split, "gemm + attention")


@pytest.mark.parametrize("H,I", [(128, 512), (512, 2048), (256, 2688), (384, 2688), (256, 192)])
def test_shapes_the_route_declines(H, I):
    """skinny_layer_supported is asked before anything is launched: -2, the entries' "not this kernel"."""
    d = _tail_inputs(8, H, I)
    with pytest.raises(RuntimeError, match="failed: -2$"):
        pybert.test_skinny_tail(*_tail_args(d, I))
    if H not in (256, 384):
        W, bias = _qkv_weights(H)
        with pytest.raises(RuntimeError, match="failed: -2$"):
            pybert.test_skinny_qkv(W.view(np.uint8), 1, bias, x=d["x"])
        with pytest.raises(RuntimeError, match="failed: -2$"):
            pybert.test_qkv_attention(d["x"], np.array([0, 8], dtype=np.int32), H // 32, 32, W.view(np.uint8), 1, bias, 5)


# ------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------
SKINNY = {"skinny_qkv", "skinny_proj", "skinny_ffn_up", "skinny_ffn_down", "skinny_layernorm", "attention"}


def _dims(H, I):
    name = f"h{H}-i{I}-l3"
    gf.MODEL_DIMS.setdefault(name, gf.BertHParams(1000, 128, H, I, H // 32, 3))
    return name


@pytest.mark.parametrize("H,I,ftype", [(256, 256, "f16"), (256, 640, "f16"), (256, 640, "q4_0"), (384, 384, "f16"), (384, 2560, "f16")])
def test_latency_route_at_the_widths_nobody_ran(make_model, H, I, ftype):
    """test_latency_route_gives_the_batch_route_s_bits at I / 128 = 2, 3, 5 and 20: a sentence alone (the route), the five
    together (264 tokens: the batch route under the suite's one-window cap) and the five together on the route give the same bits."""
    path, hp = make_model(_dims(H, I), ftype, 0)
    m = pybert.BertModel(path)
    rng = np.random.default_rng(13)
    sents = [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in [128, 25, 1, 77, 33]]
    m.profile(True)
    alone = [m.eval_batch([s])[0] for s in sents]
    names_alone = set(m.profile_report())
    batch = m.eval_batch(sents)
    names_batch = set(m.profile_report())
    m.set_option("latency_tokens", "768")
    routed = m.eval_batch(sents)
    names_routed = set(m.profile_report())
    m.profile(False)
    assert SKINNY <= names_alone and "layer_tail" not in names_alone, names_alone
    assert {"qkv_attention2", "layer_tail"} <= names_batch and not any(k.startswith("skinny") for k in names_batch), names_batch
    assert SKINNY <= names_routed and not {"layer_tail", "qkv_attention2", "model_kernel"} & names_routed, names_routed
    for i, s in enumerate(sents):
        assert np.array_equal(alone[i], batch[i]), ("alone", len(s), float(np.abs(alone[i] - batch[i]).max()))
        assert np.array_equal(routed[i], batch[i]), ("routed", len(s), float(np.abs(routed[i] - batch[i]).max()))
    assert cosine(alone[3], orc.Oracle(path).eval(sents[3])) >= TIGHT_COS_GGML[ftype]


@pytest.mark.parametrize("dims", ["minilm-l6", (256, 640)], ids=["minilm-l6", "h256-i640-l3"])
def test_hidden_tap_on_the_latency_route(make_model, dims):
    """With a hidden-state tap every layer of the route ends in skinny_layernorm, and the next layer's projection writes the same
    rows again: every layer's states and the embedding have the bits of the batch route's kernels."""
    path, hp = make_model(dims if isinstance(dims, str) else _dims(*dims), "f16", 0)
    m = pybert.BertModel(path)
    s = np.random.default_rng(17).integers(0, hp.n_vocab, size=77).astype(np.int32)
    m.profile(True)
    emb, hid = m.eval_hidden(s)
    on = m.profile_report()
    m.set_option("latency", "0")
    emb_batch, hid_batch = m.eval_hidden(s)
    off = m.profile_report()
    m.profile(False)
    assert on["skinny_layernorm"]["launches"] == hp.n_layer and on["skinny_qkv"]["launches"] == hp.n_layer, on
    assert "layer_tail" in off and not any(k.startswith("skinny") for k in off), off
    for layer in range(hp.n_layer + 1):
        assert np.array_equal(hid[layer], hid_batch[layer]), (layer, float(np.abs(hid[layer] - hid_batch[layer]).max()))
    assert np.array_equal(emb, emb_batch)
    assert np.isfinite(hid).all() and np.abs(hid[hp.n_layer]).max() > 0.1
