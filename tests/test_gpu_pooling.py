"""The pooling settings of a context (include/bert_hip.h: "pooling" = "mean" | "cls", "normalize" = "1" | "0") on the GPU: the
pooling kernel in all four combinations against float64, then every route of the forward pass against the CPU oracle's last hidden
state pooled in float64 here, the promises that carry no model tolerance (same bits alone and in a batch, on every pair of routes
that promises them, host and device entry point), the settings' own behaviour, and the index's text entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

from conftest import ROOT, cosine
from test_gpu_parity import MIN_COS

pytestmark = pytest.mark.gpu

MODES = [("mean", "1"), ("mean", "0"), ("cls", "1"), ("cls", "0")]
NEW_MODES = MODES[1:]


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _pool64(rows, pooling, normalize):
    """rows [n][H] float64 -> the sentence's embedding as the header defines it"""
    y = rows[0] if pooling == "cls" else rows.mean(axis=0)
    return y / np.sqrt((y * y).sum()) if normalize == "1" else y


# ------------------------------------------------------------------------------------------------
# the kernel, through bert_hip_test_pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 384, 768, 130])
def test_pool_kernel_modes(H):
    """The shapes of test_pool_normalize_kernel (16-byte path, 4-byte path, H no multiple of 64).  (mean, 1) keeps the bits of the
    hook that has no settings; (cls, 0) is the stored f16 row exactly; the other two against float64 on the same f16 array within
    that test's 2e-6 (set for rows of norm 1), scaled by the magnitude of an un-normalised row."""
    rng = np.random.default_rng(H)
    lens = [1, 2, 3, 5, 31, 64, 128, 300, 512]
    cu = _cu(lens)
    x = rng.normal(0.1, 1, (int(cu[-1]), H)).astype(np.float16)
    x64 = x.astype(np.float64)
    plain, st = pybert.test_pool_normalize(x, cu, 512)
    assert st == 0
    for pooling, normalize in MODES:
        got, st = pybert.test_pool(x, cu, 512, pooling, normalize == "1")
        assert st == 0, (pooling, normalize)
        if (pooling, normalize) == ("mean", "1"):
            assert np.array_equal(got, plain)
        for b, n in enumerate(lens):
            if (pooling, normalize) == ("cls", "0"):
                assert np.array_equal(got[b], x[cu[b]].astype(np.float32)), (H, n)
            else:
                want = _pool64(x64[cu[b]:cu[b + 1]], pooling, normalize)
                err = float(np.abs(got[b] - want).max())
                print(f"H {H} {pooling}/{normalize} n {n}: max error {err:.3g}, |want|.max() {np.abs(want).max():.3g}")
                assert err < 2e-6 * max(1.0, float(np.abs(want).max())), (H, pooling, normalize, n, err)
        # the length guard does not depend on the mode
        got, st = pybert.test_pool(x, cu, 128, pooling, normalize == "1")
        assert st == 1 and np.isnan(got[7]).all() and np.isnan(got[8]).all() and np.isfinite(got[:7]).all(), (pooling, normalize)


# ------------------------------------------------------------------------------------------------
# end to end, per route
# ------------------------------------------------------------------------------------------------
LENS = [1, 2, 5, 16, 17, 31, 64, 127, 128]
# test_gpu_parity.py's hidden-state tolerances per layer (test_hidden_states_match_oracle, test_f32_route_hidden_states)
HIDDEN_TOL = {"f16": 6e-3, "q4_1": 0.25, "f32": 2e-4}
# The q4 tolerance is 0.25 per layer whatever the states' size, and the synthetic weights give states of size 1: the first row and the
# mean of a sentence then differ by about 1, not by ten tolerances (7.5).  The folded arm's model has the gain of its LAST LayerNorm
# multiplied by 8, which scales the last states and nothing in front of them.
H768 = gf.BertHParams(2000, 64, 768, 3072, 12, 2)
H768_LAST_GAIN = 8.0
# model: (dims | None for H768, ftype, seed of the weights, seed of the ids).  minilm: of the weight seeds 0 .. 23, 6 is the first whose
# two-token sentence ([CLS] [SEP], whatever the ids' seed) has the gap the precondition below asks for (0.505 against 0.42); the ids'
# seed 100 leaves every sentence above 0.5.
MODELS = {"minilm": ("minilm-l6", "f16", 6, 100), "h768": (None, "q4_1", 1, 500), "tiny": ("tiny", "f32", 0, 500)}
# arm: (model, options, kernels that the default mode's profile must show, kernels that it must not)
ARMS = {
    "one_launch": ("minilm", {"one_launch": "2"}, {"model_kernel"}, {"qkv_attention2", "layer_tail", "pool_normalize"}),
    "fused": ("minilm", {"one_launch": "0", "latency": "0"}, {"qkv_attention2", "layer_tail", "pool_normalize"}, {"model_kernel", "skinny_qkv"}),
    # (tests run with BERT_HIP_LATENCY=128, conftest.py: the shipped cap is set here, as the tests of the route itself do)
    "latency": ("minilm", {"one_launch": "0", "latency_tokens": "768"}, {"skinny_qkv", "pool_normalize"}, {"model_kernel", "layer_tail"}),
    "tiled": ("minilm", {"qkv2": "0", "tail": "0", "latency": "0", "one_launch": "0"}, {"gemm_qkv", "attention", "layernorm", "pool_normalize"},
              {"model_kernel", "qkv_attention2", "layer_tail", "skinny_qkv"}),
    "folded": ("h768", {}, {"ln_rows_finalize", "pool_normalize"}, {"model_kernel", "layer_tail"}),
    "f32": ("tiny", {}, {"family:gemm_f32", "pool_normalize"}, {"family:gemm_mfma_f16", "family:gemm256_f16"}),
}


def _model_file(name, make_model, model_dir):
    dims, ftype, seed, _ = MODELS[name]
    if dims is not None:
        return make_model(dims, ftype, seed)
    path = os.path.join(model_dir, f"pooling_h768_{ftype}_s{seed}.bin")
    if not os.path.exists(path):
        w = gf.synthetic_weights(H768, seed)
        w[f"encoder.layer.{H768.n_layer - 1}.output.LayerNorm.weight"] *= np.float32(H768_LAST_GAIN)
        gf.write_model(path, H768, w, gf.FTYPE_BY_NAME[ftype])
    return path, H768


def _sentences(name, hp):
    """the batch of the issue: lengths LENS, capped by the model's position table; ids from synthetic_token_ids"""
    return [gf.synthetic_token_ids(1, min(n, hp.n_max_tokens), hp.n_vocab, seed=MODELS[name][3] + i)[0] for i, n in enumerate(LENS)]


_REF = {}


def reference(name, make_model, model_dir):
    """(path, hparams, sentences, {mode: [B][H] float64}): the oracle's last hidden state pooled in float64, computed once per model.
    Asserts the precondition on the oracle alone: for every sentence of two tokens or more the first row and the mean differ, in
    some element, by more than ten times the un-normalised tolerance — no arm can pass a mode's comparison with another mode's rows."""
    if name not in _REF:
        path, hp = _model_file(name, make_model, model_dir)
        sents = _sentences(name, hp)
        o = orc.Oracle(path)
        last = [o.eval(s, orc.MODE_PLAIN, want_hidden=True)[1][-1].astype(np.float64) for s in sents]
        tol = HIDDEN_TOL[MODELS[name][1]] * (1 + hp.n_layer)
        for s, rows in zip(sents, last):
            assert rows.shape == (len(s), hp.n_embd)
            if len(s) >= 2:
                gap = float(np.abs(rows[0] - rows.mean(axis=0)).max())
                assert gap > 10 * tol, (name, len(s), gap, tol)
        _REF[name] = (path, hp, sents, {mode: np.stack([_pool64(rows, *mode) for rows in last]) for mode in MODES})
    return _REF[name]


class _Hip:
    """hipMalloc / hipMemcpy of the runtime libbert.so is linked against, for the device entry point"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(arr.nbytes)) == 0
        assert self.lib.hipMemcpy(p, C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0
        return p.value

    def download(self, p, shape):
        out = np.empty(shape, dtype=np.float32)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self, *ptrs):
        for p in ptrs:
            assert self.lib.hipFree(C.c_void_p(p)) == 0


def _set_mode(m, mode):
    m.set_option("pooling", mode[0])
    m.set_option("normalize", mode[1])
    assert (m.pooling(), m.normalize()) == (int(mode[0] == "cls"), int(mode[1])), mode


_RUNS = {}


def run_arm(arm, make_model, model_dir):
    """Everything one context of the arm computes, once: per mode the batch through the host entry point, every sentence alone, the
    device entry point and bert_hip_eval_hidden's embedding; what a bad value and the way back to the defaults leave behind."""
    if arm in _RUNS:
        return _RUNS[arm]
    name, options, must, must_not = ARMS[arm]
    path, hp, sents, _ = reference(name, make_model, model_dir)
    toks, cu = np.concatenate(sents).astype(np.int32), _cu([len(s) for s in sents])
    B, T, H, max_len = len(sents), int(cu[-1]), hp.n_embd, max(len(s) for s in sents)
    hip = _Hip()
    m = pybert.BertModel(path)
    for k, v in options.items():
        m.set_option(k, v)
    assert (m.pooling(), m.normalize()) == (0, 1)
    r = {"host": {}, "alone": {}, "device": {}, "hidden": {}}
    r["host"][MODES[0]] = m.eval_packed(toks, cu)
    m.profile(True)
    r["profiled"] = m.eval_packed(toks, cu)
    names = set(m.profile_report(families=True))
    m.profile(False)
    assert must <= names and not must_not & names, (arm, sorted(names))
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.upload(np.zeros((B, H), np.float32))
    m.reserve(T, B)
    for mode in NEW_MODES:
        _set_mode(m, mode)
        r["host"][mode] = m.eval_packed(toks, cu)
        r["alone"][mode] = np.stack([m.eval_packed(s, [0, len(s)])[0] for s in sents])
        m.eval_packed_device(d_t, d_cu, B, T, max_len, d_out, 0)
        assert m.check() == 0
        r["device"][mode] = hip.download(d_out, (B, H))
        r["hidden"][mode] = [m.eval_hidden(s) for s in (sents[2], sents[-1])]
    r["eval_batch"] = m.eval_batch(sents)                    # (bert.h's entry point, in the last mode: cls, 0)
    # a value the key does not know: a line on stderr, the setting and the rows stay
    m.set_option("pooling", "max")
    m.set_option("normalize", "yes")
    r["after_bad_value"] = (m.pooling(), m.normalize(), m.eval_packed(toks, cu))
    _set_mode(m, MODES[0])
    r["default_again"] = m.eval_packed(toks, cu)
    hip.free(d_t, d_cu, d_out)
    m.close()
    _RUNS[arm] = r
    return r


@pytest.mark.parametrize("arm", list(ARMS))
def test_route_matches_the_oracle_in_every_mode(arm, make_model, model_dir):
    name = ARMS[arm][0]
    _, hp, sents, want = reference(name, make_model, model_dir)
    ftype = MODELS[name][1]
    r = run_arm(arm, make_model, model_dir)
    tol = HIDDEN_TOL[ftype] * (1 + hp.n_layer)
    for mode in MODES:
        got = r["host"][mode].astype(np.float64)
        assert np.isfinite(got).all(), (arm, mode)
        for b, s in enumerate(sents):
            if mode[1] == "1":
                c = cosine(got[b], want[mode][b])
                print(f"{arm} {mode} n {len(s)}: cosine {c:.9f}")
                assert c > MIN_COS[ftype], (arm, mode, len(s), c)
                assert abs(np.linalg.norm(got[b]) - 1) < 1e-5, (arm, mode, len(s))
            else:
                err = float(np.abs(got[b] - want[mode][b]).max())
                print(f"{arm} {mode} n {len(s)}: max error {err:.3g} (bound {tol:.3g})")
                assert err < tol, (arm, mode, len(s), err, tol)
    # ties to the default mode's rows, which carry no model tolerance: an un-normalised row divided by its float64 norm is the
    # normalised one
    for raw, normed in ((("mean", "0"), ("mean", "1")), (("cls", "0"), ("cls", "1"))):
        y = r["host"][raw].astype(np.float64)
        y /= np.sqrt((y * y).sum(axis=1, keepdims=True))
        err = float(np.abs(y - r["host"][normed]).max())
        assert err < 2e-6, (arm, raw, err)


@pytest.mark.parametrize("arm", list(ARMS))
def test_same_bits_alone_in_the_batch_and_through_the_device_entry_point(arm, make_model, model_dir):
    r = run_arm(arm, make_model, model_dir)
    assert np.array_equal(r["profiled"], r["host"][MODES[0]])
    for mode in NEW_MODES:
        neq = np.argwhere((r["alone"][mode] != r["host"][mode]).any(axis=1)).ravel().tolist()
        assert not neq, (arm, mode, "alone vs batch, sentences", neq)
        assert np.array_equal(r["device"][mode], r["host"][mode]), (arm, mode, "device vs host entry point")
        # the embedding bert_hip_eval_hidden returns follows the setting; under (cls, 0) it is the tap's first row of the last layer
        for emb, hid in r["hidden"][mode]:
            if mode == ("cls", "0"):
                assert np.array_equal(emb, hid[-1][0]), (arm, mode)
            else:
                want = _pool64(hid[-1].astype(np.float64), *mode)
                assert np.abs(emb - want).max() < 2e-6 * max(1.0, float(np.abs(want).max())), (arm, mode)
    assert np.array_equal(r["eval_batch"], r["host"][("cls", "0")])


@pytest.mark.parametrize("a,b", [("one_launch", "fused"), ("latency", "fused")])
def test_routes_that_promise_the_same_bits_keep_them_in_every_mode(a, b, make_model, model_dir):
    ra, rb = run_arm(a, make_model, model_dir), run_arm(b, make_model, model_dir)
    for mode in MODES:
        assert np.array_equal(ra["host"][mode], rb["host"][mode]), (a, b, mode)


def test_full_windows_in_one_launch_keep_the_two_kernel_bits(make_model, model_dir):
    """Sentences of exactly 128 tokens take model_kernel's form for full windows (the issue's batch is ragged): its epilogue is the same body."""
    path, hp, _, _ = reference("minilm", make_model, model_dir)
    ids = gf.synthetic_token_ids(3, 128, hp.n_vocab, seed=321)
    toks, cu = ids.reshape(-1), _cu([128] * 3)
    rows = {}
    for arm in ("one_launch", "fused"):
        m = pybert.BertModel(path)
        for k, v in ARMS[arm][1].items():
            m.set_option(k, v)
        m.profile(True)
        for mode in MODES:
            _set_mode(m, mode)
            rows[arm, mode] = m.eval_packed(toks, cu)
        assert ("model_kernel" in m.profile_report()) == (arm == "one_launch")
        m.close()
    for mode in MODES:
        assert np.array_equal(rows["one_launch", mode], rows["fused", mode]), mode
    assert np.array_equal(rows["fused", ("cls", "0")][1], rows["fused", ("cls", "0")][1].astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("arm", list(ARMS))
def test_settings_bad_value_and_the_way_back(arm, make_model, model_dir):
    r = run_arm(arm, make_model, model_dir)
    pooling, normalize, rows = r["after_bad_value"]
    assert (pooling, normalize) == (1, 0) and np.array_equal(rows, r["host"][("cls", "0")]), arm
    assert np.array_equal(r["default_again"], r["host"][MODES[0]]), arm


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from bert_cpp_amd import pybert
z = np.load(sys.argv[3])
m = pybert.BertModel(sys.argv[2])
assert (m.pooling(), m.normalize()) == (1, 0), (m.pooling(), m.normalize())
np.save(sys.argv[4], m.eval_packed(z["toks"], z["cu"]))
m.close()
os.environ["BERT_HIP_POOLING"] = "max"            # a value the variable does not know: a line on stderr, the default stays
m = pybert.BertModel(sys.argv[2])
assert (m.pooling(), m.normalize()) == (0, 0), (m.pooling(), m.normalize())
"""


def test_environment_at_load_equals_the_keys(make_model, model_dir, tmp_path):
    """BERT_HIP_POOLING / BERT_HIP_NORMALIZE are read by bert_load_from_file: a fresh process."""
    path, _, sents, _ = reference("minilm", make_model, model_dir)
    batch, out = str(tmp_path / "batch.npz"), str(tmp_path / "rows.npy")
    np.savez(batch, toks=np.concatenate(sents).astype(np.int32), cu=_cu([len(s) for s in sents]))
    env = dict(os.environ, BERT_HIP_POOLING="cls", BERT_HIP_NORMALIZE="0")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, path, batch, out], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "pooling" in p.stderr and "max" in p.stderr
    assert np.array_equal(np.load(out), run_arm("fused", make_model, model_dir)["host"][("cls", "0")])


def test_index_text_entry_points_follow_the_setting(make_model, model_dir):
    path, _, _, _ = reference("minilm", make_model, model_dir)
    with open(os.path.join(ROOT, "tests", "golden", "sample_client_texts_600.txt"), encoding="utf-8") as f:
        texts = [line.rstrip("\n") for line in f][:40]
    queries = ["Should I get health insurance?", "poaching", texts[7], texts[23]]
    m = pybert.BertModel(path)
    mean_rows = m.encode_batch(texts)
    _set_mode(m, ("cls", "1"))
    rows, q = m.encode_batch(texts), m.encode_batch(queries)
    assert np.isfinite(rows).all() and not np.array_equal(rows, mean_rows)
    a, b = m.index(dtype="f32"), m.index(dtype="f32")
    assert a.add_texts(texts) == 0
    b.add(rows)
    ia, sa = a.search_texts(queries, 5)
    ib, sb = b.search(q, 5)
    assert np.array_equal(ia, ib) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
    assert (ia >= 0).all()
    m.close()
