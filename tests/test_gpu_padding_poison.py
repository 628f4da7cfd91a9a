"""The batch route's kernels compute whole tiles of 128 or 256 tokens, and the engine's workspaces are grow-only: behind a call's last
token, and wherever a pass has not written yet, they hold what an earlier pass left.  No result may depend on that.

Op level (include/bert_hip_test.h, bert_hip_test_set_pad): every batch-route entry with zeros and with quiet NaNs in the padding rows of
its inputs and in every word of its output and intermediate buffers -- equal bits, no NaN, and the prefix property: rows 0 .. M - 1
of an M-row call have the bits of the same rows in a 257-row call (attention: a sentence has the same bits when other sentences
follow it).  M runs over the edges of the 32-, 128- and 256-token tiles; every result is also held to the float64 check and the
tolerance test_gpu_parity.py asserts for its kernel.

Model level ("test_poison_workspace" of libbert_test.so's engine, options.h): on every route, a batch, the same batch after every
activation workspace became NaN, and -- poisoned again -- a three-sentence prefix of it against a fresh context."""
import functools

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import layer_reference as ref
from test_gpu_latency_kernels import NAN16, NAN32, SKINNY, _same_bits
from test_gpu_parity import Q2_CASES, WT, _attention_ref, _q4_image_f16, _weight_bytes

pytestmark = pytest.mark.gpu

TOKENS = [1, 2, 31, 33, 127, 128, 129, 255, 256, 257]
BIG = 257


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


def _clean_and_poisoned(run, what):
    """run() with zeros and with quiet NaNs where the engine would have stale data: the same bits, and no NaN in them."""
    clean = _tuple(run())
    with pybert.test_pad(NAN16, NAN32):
        dirty = _tuple(run())
    for i, (a, b) in enumerate(zip(clean, dirty)):
        assert not np.isnan(b).any(), (what, i, "NaN padding reached rows", np.unique(np.argwhere(np.isnan(b))[:, 0])[:8].tolist())
        assert not np.isnan(a).any(), (what, i)
        _same_bits(b, a, f"{what}: output {i}, NaN against zero padding")
    return clean


# ------------------------------------------------------------------------------------------------
# mat-muls
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _gemm_inputs(N, K, ftype):
    """test_gemm_kernel's distributions, 257 rows"""
    rng = np.random.default_rng(7 * N + K + WT[ftype])
    A = rng.normal(0, 1, (BIG, K)).astype(np.float16)
    W = (rng.normal(0, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    W[:, : K // 2] *= 1.5
    W[: N // 3] += 0.02
    bias = rng.normal(0, 0.5, N).astype(np.float32)
    resid = rng.normal(0, 1, (BIG, N)).astype(np.float16)
    wb, wdeq = _weight_bytes(W, ftype)
    base = ref.f8(A) @ ref.f8(wdeq).T + bias
    return A, wb, bias, resid, base


def _gemm_token_edges(impl, N, K, ftype):
    A, wb, bias, resid, base = _gemm_inputs(N, K, ftype)
    for epi in (0, 1, 2):
        want = base if epi == 0 else ref.gelu(base) if epi == 1 else base + ref.f8(resid)
        run = lambda M: pybert.test_gemm(A[:M], wb, WT[ftype], N, bias, resid[:M] if epi == 2 else None, epi, impl)
        big, = _clean_and_poisoned(lambda: run(BIG), (impl, epi, BIG))
        for M in TOKENS:
            got, = _clean_and_poisoned(lambda: run(M), (impl, epi, M))
            _same_bits(got, big[:M], f"impl {impl} epilogue {epi}: {M} rows against the first rows of {BIG}")
            err = np.abs(ref.f8(got) - want[:M])
            bad = err > 2e-3 * np.abs(want[:M]) + 4e-3            # (test_gemm_kernel's tolerance)
            assert not bad.any(), (impl, epi, M, int(bad.sum()), float(err.max()), np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("impl", [0, 1], ids=["mfma", "naive"])
@pytest.mark.parametrize("ftype", ["f16", "q4_0", "q4_1"])
@pytest.mark.parametrize("N,K", [(64, 64), (192, 128), (384, 384)])
def test_gemm_rows_do_not_depend_on_the_padding(impl, ftype, N, K):
    """gemm.hip's 128 x 128 kernel (q4 blocks expanded in the tile load) and the generic kernel, all three epilogues: a partial
    feature tile, one and several reduction tiles."""
    _gemm_token_edges(impl, N, K, ftype)


@pytest.mark.parametrize("ftype", ["f16", "q4_0", "q4_1"])
@pytest.mark.parametrize("N,K", [(256, 128), (768, 256)])
def test_gemm256_rows_do_not_depend_on_the_padding(ftype, N, K):
    """gemm256.hip: 256-token tiles (one token can bring 255 padding rows), the minimum of two reduction tiles, three feature tiles."""
    _gemm_token_edges(3, N, K, ftype)


@functools.lru_cache(maxsize=1)
def _lnfold_inputs(K1, H, N2):
    """test_layernorm_folded_into_the_gemms' distributions, 257 rows"""
    rng = np.random.default_rng(K1 + H + N2)
    d = dict(A1=rng.normal(0, 1, (BIG, K1)).astype(np.float16), W1=(rng.normal(0, 1, (H, K1)) / np.sqrt(K1)).astype(np.float16),
             b1=rng.normal(0, 0.3, H).astype(np.float32), r=(rng.normal(0, 1, (BIG, H)) + rng.normal(0, 0.7, (BIG, 1))).astype(np.float16),
             rg=(1 + rng.normal(0, 0.2, H)).astype(np.float32), rb=rng.normal(0, 0.2, H).astype(np.float32),
             W2=(rng.normal(0, 1, (N2, H)) / np.sqrt(H)).astype(np.float16), b2=rng.normal(0, 0.5, N2).astype(np.float32),
             g=(1 + rng.normal(0, 0.2, H)).astype(np.float32), be=rng.normal(0, 0.3, H).astype(np.float32))
    return d


@pytest.mark.parametrize("epi2", [0, 1], ids=["bias", "gelu"])
@pytest.mark.parametrize("rebuild", [False, True], ids=["plain-residual", "rebuilt-residual"])
def test_lnfold_rows_do_not_depend_on_the_padding(rebuild, epi2, K1=128, H=256, N2=512):
    """The LayerNorm fold's pair of mat-muls: the partial statistics, ln_rows_finalize over all 256 rows of the tile and the row
    scale of the consuming mat-mul, with NaN residual rows (and NaN row statistics of the residual) behind the last token."""
    d = _lnfold_inputs(K1, H, N2)
    rg, rb = (d["rg"], d["rb"]) if rebuild else (None, None)
    run = lambda M: pybert.test_gemm_lnfold(d["A1"][:M], d["W1"], d["b1"], d["r"][:M], rg, rb, d["W2"], d["b2"], d["g"], d["be"], epi2)
    big = _clean_and_poisoned(lambda: run(BIG), (rebuild, epi2, BIG))
    resid = ref.layernorm(ref.f8(d["r"]), ref.f8(d["rg"]), ref.f8(d["rb"])) if rebuild else ref.f8(d["r"])
    u_ref = ref.f8(d["A1"]) @ ref.f8(d["W1"]).T + d["b1"] + resid
    for M in TOKENS:
        got = _clean_and_poisoned(lambda: run(M), (rebuild, epi2, M))
        for name, a, b in zip(("u", "out", "rows"), got, big):
            _same_bits(a, b[:M], f"{name}: {M} rows against the first rows of {BIG}")
        # test_layernorm_folded_into_the_gemms' float64 checks and tolerances
        u, out, rows = got
        err = np.abs(ref.f8(u) - u_ref[:M])
        assert not (err > 2e-3 * np.abs(u_ref[:M]) + 6e-3).any(), ("u", M, float(err.max()))
        uf = ref.f8(u)
        mu, sd = uf.mean(axis=1), np.sqrt(uf.var(axis=1) + 1e-5)
        assert np.abs(rows[:, 3] - sd).max() < 2e-5 * sd.max() + 1e-6 and np.abs(-rows[:, 2] - mu).max() < 1e-5, M
        base = ref.layernorm(uf, ref.f8(d["g"]), ref.f8(d["be"])) @ ref.f8(d["W2"]).T + d["b2"]
        want = ref.gelu(base) if epi2 == 1 else base
        err = np.abs(ref.f8(out) - want)
        assert not (err > 3e-3 * np.abs(want) + 8e-3).any(), ("out", M, float(err.max()))
        assert err.mean() < 6e-4, (M, float(err.mean()))


# ------------------------------------------------------------------------------------------------
# layer tail
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tail_inputs(H, I, ftype):
    """test_layer_tail_kernel's distributions (test_layer_tail_kernel_q4's for q4 blocks), 257 rows; the float64 reference on the f16
    image of the weights the device computes with"""
    rng = np.random.default_rng(H + I + WT[ftype])
    ctx = rng.normal(0, 1, (BIG, H)).astype(np.float16)
    x = rng.normal(0, 1, (BIG, H)).astype(np.float16)
    Ws = [(rng.normal(0, 1, shp) / np.sqrt(shp[1])).astype(np.float32) for shp in ((H, H), (I, H), (H, I))]
    if ftype == "f16":
        imgs = [w.astype(np.float16) for w in Ws]
        wbs = [w.view(np.uint8) for w in imgs]
    else:
        qs = [gf.quantize_q4_0(w) for w in Ws]
        imgs = [_q4_image_f16(q, WT[ftype], w.shape) for q, w in zip(qs, Ws)]
        wbs = [q.view(np.uint8) for q in qs]
    f4 = lambda a: a.astype(np.float32)
    bo, b2 = f4(rng.normal(0, 0.2, H)), f4(rng.normal(0, 0.2, H))
    b1 = f4(rng.normal(0, 0.5, I))
    g1, g2 = f4(1 + rng.normal(0, 0.1, H)), f4(1 + rng.normal(0, 0.1, H))
    be1, be2 = f4(rng.normal(0, 0.1, H)), f4(rng.normal(0, 0.1, H))
    params = (bo, g1, be1, b1, b2, g2, be2)
    want = ref.layer_tail(ctx, x, *imgs, *[ref.f8(p) for p in params])
    return ctx, x, wbs, params, want


@pytest.mark.parametrize("H,I,ftype,impl", [(256, 256, "f16", 1), (256, 256, "q4_0", 1), (384, 256, "f16", 1), (384, 256, "q4_0", 1),
                                            (128, 128, "f16", 0)])
def test_layer_tail_rows_do_not_depend_on_the_padding(H, I, ftype, impl):
    """layer_tail.hip (a pair of specialist waves per 32 tokens of a 128-token tile) and the five kernels of the shapes it does not
    take (there y and the intermediate pass through buffers that hold NaN before the first launch)."""
    ctx, x, wbs, params, want = _tail_inputs(H, I, ftype)
    run = lambda M: pybert.test_layer_tail(ctx[:M], x[:M], *wbs, WT[ftype], I, *params, impl)
    big, = _clean_and_poisoned(lambda: run(BIG), (impl, BIG))
    for M in TOKENS:
        got, = _clean_and_poisoned(lambda: run(M), (impl, M))
        _same_bits(got, big[:M], f"{M} rows against the first rows of {BIG}")
        err = np.abs(ref.f8(got) - want[:M])
        assert err.max() < 2.5e-2 and err.mean() < 2e-3, (M, float(err.max()), float(err.mean()))       # (test_layer_tail_kernel's)


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
FOLLOWERS = [33, 128, 5]


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@pytest.mark.parametrize("impl", [0, 1], ids=["mfma", "naive"])
@pytest.mark.parametrize("d_head,n_head", [(32, 3), (64, 2)])
@pytest.mark.parametrize("lens", [[1], [17, 1, 128], [129], [300, 7]], ids=lambda l: "-".join(map(str, l)))
def test_attention_rows_do_not_depend_on_the_padding(impl, d_head, n_head, lens):
    """attention.hip pads a sentence's K and V^T to whole key tiles in LDS: the rows of qkv behind the LAST sentence are what it would
    find there if it loaded them (P is 0 there, and 0 x NaN is NaN).  test_attention_kernel's distributions and tolerance."""
    H = n_head * d_head
    rng = np.random.default_rng(sum(lens) + d_head)
    more = lens + FOLLOWERS
    cu, cu_more = _cu(lens), _cu(more)
    T = int(cu[-1])
    qkv = rng.normal(0, 1, (int(cu_more[-1]), 3 * H)).astype(np.float16)
    qkv[:, :H] *= 1.7
    for b in range(len(more)):
        qkv[cu_more[b + 1] - 1, H:2 * H] *= 4.0
    got, = _clean_and_poisoned(lambda: pybert.test_attention(qkv[:T], cu, n_head, d_head, impl), (impl, lens))
    followed, = _clean_and_poisoned(lambda: pybert.test_attention(qkv, cu_more, n_head, d_head, impl), (impl, more))
    _same_bits(got, followed[:T], "sentences alone against the same sentences with others behind them")
    err = np.abs(ref.f8(followed) - _attention_ref(qkv, cu_more, n_head, d_head))
    assert err.max() < 6e-3, (impl, d_head, lens, float(err.max()), np.argwhere(err > 6e-3)[:5].tolist())


@pytest.mark.parametrize("mode", [2, 3, 4], ids=["next-fit", "uniform", "next-fit-on-device"])
@pytest.mark.parametrize("n_head", [4, 8, 12])
@pytest.mark.parametrize("case", [1, 4, 5])
def test_qkv_attention2_rows_do_not_depend_on_the_padding(n_head, case, mode):
    """qkv_attention2.hip: the slots of a window between and behind its sentences read the window's first token, not their own row
    of x (behind the last sentence: NaN here).  test_qkv_attention2_kernel's distributions, tolerance and equal-bits check."""
    lens = Q2_CASES[case]
    d_head, H = 32, 32 * n_head
    rng = np.random.default_rng(sum(lens) + n_head)
    more = lens + FOLLOWERS
    cu, cu_more = _cu(lens), _cu(more)
    T = int(cu[-1])
    x = rng.normal(0, 1, (int(cu_more[-1]), H)).astype(np.float16)
    W = (rng.normal(0, 1, (3 * H, H)) / np.sqrt(H)).astype(np.float16)
    W[:H] *= 1.7
    W[:, : H // 2] *= 1.3
    bias = rng.normal(0, 0.3, 3 * H).astype(np.float32)
    run = lambda rows, c, m: pybert.test_qkv_attention(rows, c, n_head, d_head, W.view(np.uint8), 1, bias, m)
    got, = _clean_and_poisoned(lambda: run(x[:T], cu, mode), (mode, "alone"))
    followed, = _clean_and_poisoned(lambda: run(x, cu_more, mode), (mode, "followed"))
    split, = _clean_and_poisoned(lambda: run(x, cu_more, 0), (0, "followed"))
    _same_bits(got, followed[:T], "sentences alone against the same sentences with others behind them")
    _same_bits(followed, split, "window kernel against mat-mul + attention kernel")
    qkv = (ref.f8(x) @ ref.f8(W).T + bias).astype(np.float16)
    err = np.abs(ref.f8(followed) - _attention_ref(qkv, cu_more, n_head, d_head))
    assert err.max() < 6e-3, (n_head, mode, float(err.max()), np.argwhere(err > 6e-3)[:8].tolist())


# ------------------------------------------------------------------------------------------------
# whole models
# ------------------------------------------------------------------------------------------------
LENS = [128, 1, 17, 33, 64, 127, 5, 128, 96]
TWO_KERNELS = {"qkv_attention2", "layer_tail"}
TILED = {"gemm_qkv", "attention", "gemm_attn_out", "layernorm", "gemm_ffn_up", "gemm_ffn_down"}

# id -> (dims, ftype, lens, environment at load, options, kernels that must run, kernels that must not)
ROUTES = {
    "one-launch-full": ("minilm-l6", "f16", [128] * 9, {}, {"latency": "0", "one_launch": "2"}, {"model_kernel"}, TWO_KERNELS | SKINNY),
    "one-launch-ragged": ("minilm-l6", "f16", LENS, {}, {"latency": "0", "one_launch": "2"}, {"model_kernel"}, TWO_KERNELS | SKINNY),
    "two-kernels": ("minilm-l6", "f16", LENS, {}, {"latency": "0", "one_launch": "0"}, TWO_KERNELS, {"model_kernel"} | SKINNY),
    "tiled": ("minilm-l6", "f16", LENS, {"BERT_HIP_KERNELS": "tiled"}, {}, TILED, TWO_KERNELS | {"model_kernel"} | (SKINNY - {"attention"})),
    "latency": ("minilm-l6", "f16", LENS, {}, {"latency_tokens": "768"}, SKINNY, TWO_KERNELS | {"model_kernel"}),
    "q4-fused": ("minilm-l6", "q4_0", LENS, {"BERT_HIP_Q4": "fused"}, {"latency": "0"}, TWO_KERNELS, {"gemm_qkv"}),
    "h256-one-launch": ("h256-l3", "f16", LENS, {}, {"latency": "0", "one_launch": "2"}, {"model_kernel"}, TWO_KERNELS | SKINNY),
    "bert-base-fold": ("bert-base-l2", "f16", LENS + [300], {"BERT_HIP_LN_FOLD": "1"}, {}, TILED | {"ln_rows_finalize"}, TWO_KERNELS),
    "bert-base-plain": ("bert-base-l2", "f16", LENS + [300], {"BERT_HIP_LN_FOLD": "0"}, {}, TILED, TWO_KERNELS | {"ln_rows_finalize"}),
    "bert-base-q4_1": ("bert-base-l2", "q4_1", LENS + [300], {}, {}, TILED, TWO_KERNELS),
    "f32": ("tiny", "f32", LENS, {}, {}, TILED | {"family:gemm_f32"}, {"family:gemm_mfma_f16", "family:gemm256_f16", "family:gemm_naive"}),
}


def _load(path, env, options, monkeypatch):
    with monkeypatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        m = pybert.BertModel(path, test_routes=True)          # (libbert_test.so: the engine that knows "test_poison_workspace")
    for k, v in options.items():
        m.set_option(k, v)
    return m


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_no_route_reads_what_an_earlier_pass_left(make_model, route, monkeypatch):
    """A batch X; every activation workspace NaN; X again: equal bits.  Poisoned again, the three-sentence prefix Y of X -- now the rows
    behind Y's last token are NaN where X's were, and so is every row a kernel of the pass has yet to write -- against Y on a
    fresh context of the same file and options.  The profiler's kernel names say that the route meant is the route that ran."""
    dims, ftype, lens, env, options, must, must_not = ROUTES[route]
    gf.MODEL_DIMS.setdefault("h256-l3", gf.BertHParams(1000, 128, 256, 1024, 8, 3))
    gf.MODEL_DIMS.setdefault("bert-base-l2", gf.BertHParams(30522, 512, 768, 3072, 12, 2))
    path, hp = make_model(dims, ftype, 0)
    rng = np.random.default_rng(5)
    X = [rng.integers(0, hp.n_vocab, size=min(n, hp.n_max_tokens)).astype(np.int32) for n in lens]
    Y = X[:3]
    m = _load(path, env, options, monkeypatch)
    m.profile(True)
    first = m.eval_batch(X)
    names = set(m.profile_report(families=True))
    m.profile(False)
    assert must <= names and not must_not & names, (route, sorted(names))
    assert np.isfinite(first).all()
    m.set_option("test_poison_workspace", "1")
    again = m.eval_batch(X)
    assert np.isfinite(again).all(), (route, "sentences with NaN", np.unique(np.argwhere(~np.isfinite(again))[:, 0]).tolist())
    assert np.array_equal(again, first), (route, float(np.abs(again - first).max()))
    m.set_option("test_poison_workspace", "1")
    prefix = m.eval_batch(Y)
    fresh = _load(path, env, options, monkeypatch)
    want = fresh.eval_batch(Y)
    assert np.isfinite(prefix).all(), (route, "sentences with NaN", np.unique(np.argwhere(~np.isfinite(prefix))[:, 0]).tolist())
    assert np.array_equal(prefix, want), (route, float(np.abs(prefix - want).max()))
    m.close(); fresh.close()


def test_hidden_state_tap_reads_nothing_an_earlier_pass_left(make_model, monkeypatch):
    """bert_hip_eval_hidden on the batch kernels (a tap behind every layer: neither the one-launch kernel nor the latency route's
    shortcut): 77 tokens twice around a poisoning, then 33 tokens against a fresh context."""
    path, hp = make_model("minilm-l6", "f16", 0)
    rng = np.random.default_rng(6)
    long, short = (rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in (77, 33))
    m = _load(path, {}, {"latency": "0"}, monkeypatch)
    m.profile(True)
    emb, hid = m.eval_hidden(long)
    names = set(m.profile_report())
    m.profile(False)
    assert TWO_KERNELS <= names and not SKINNY - {"attention"} & names and "model_kernel" not in names, sorted(names)
    m.set_option("test_poison_workspace", "1")
    emb2, hid2 = m.eval_hidden(long)
    assert np.isfinite(hid2).all() and np.array_equal(hid2, hid) and np.array_equal(emb2, emb)
    m.set_option("test_poison_workspace", "1")
    emb3, hid3 = m.eval_hidden(short)
    fresh = _load(path, {}, {"latency": "0"}, monkeypatch)
    emb4, hid4 = fresh.eval_hidden(short)
    assert np.isfinite(hid3).all() and np.array_equal(hid3, hid4) and np.array_equal(emb3, emb4)
    m.close(); fresh.close()
