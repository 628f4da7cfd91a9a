"""CPU-side tests of the cross-encoder feature (bert_hip.h "sentence pairs and scores"): the optional classification head in the model
file, pair tokenization, the float64 reference model against HuggingFace, and the head's error bound against an f32 emulation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert as libbert

import cross_encoder_reference as cer

FTYPES = ["f32", "f16", "q4_0", "q4_1"]


def _write(path, hp, w, ftype, **kw):
    gf.write_model(str(path), hp, w, gf.FTYPE_BY_NAME[ftype], **kw)
    return str(path)


def _digest_error(path, capfd):
    with pytest.raises(RuntimeError):
        libbert.model_digest(path)
    return capfd.readouterr().err


# ------------------------------------------------------------------------------------------------
# file format
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ftype", FTYPES)
@pytest.mark.parametrize("n_labels", [1, 3, 8])
def test_head_file_round_trips_and_loads(tmp_path, ftype, n_labels):
    """A file with a head reads back through ggml_file with every tensor, the head's behind the encoder's; the product's parser
    accepts it (4 tensors more); the same seed without a head gives the same encoder tensors and an unchanged digest."""
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 3, n_labels=n_labels)
    w0 = gf.synthetic_weights(hp, 3)
    assert all(np.array_equal(w[n], w0[n]) for n in w0) and set(w) - set(w0) == set(gf.HEAD_NAMES)
    with_head, without = _write(tmp_path / "h.bin", hp, w, ftype), _write(tmp_path / "n.bin", hp, w0, ftype)
    mf = gf.read_model(with_head)
    assert list(mf.raw)[-4:] == gf.HEAD_NAMES and len(mf.raw) == 5 + 16 * hp.n_layer + 4
    ft = gf.FTYPE_BY_NAME[ftype]
    assert mf.raw["pooler.dense.weight"][:2] == (ft, (hp.n_embd, hp.n_embd)) and mf.raw["classifier.weight"][:2] == (ft, (n_labels, hp.n_embd))
    assert mf.raw["pooler.dense.bias"][:2] == (0, (hp.n_embd,)) and mf.raw["classifier.bias"][:2] == (0, (n_labels,))
    tol = {"f32": 0, "f16": 1e-3, "q4_0": 0.2, "q4_1": 0.2}[ftype]
    for n in gf.HEAD_NAMES:
        assert np.abs(mf.dequantized(n) - w[n]).max() <= tol * max(1.0, np.abs(w[n]).max())
    n1, leg1, d1 = libbert.model_digest(with_head)
    n0, leg0, d0 = libbert.model_digest(without)
    assert (n1, leg1) == (5 + 16 * hp.n_layer + 4, False) and (n0, leg0) == (5 + 16 * hp.n_layer, False) and d0 != d1
    # the head-less file's digest: what the parser gave before it knew a head (FNV-1a over name, type, bytes in name order)
    raw0 = gf.read_model(without).raw
    h = 1469598103934665603
    for name in sorted(raw0):
        t, _, data = raw0[name]
        for chunk in (name.encode(), np.int32(t).tobytes(), data):
            for byte in chunk:
                h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert h == d0


def test_head_file_refusals(tmp_path, capfd):
    """A partial head, a wrong shape, n_labels 9 and another unknown name are refused, each with its message."""
    hp = gf.MODEL_DIMS["tiny"]
    H = hp.n_embd
    w = gf.synthetic_weights(hp, 1, n_labels=3)
    good = _write(tmp_path / "good.bin", hp, w, "f16")
    data = open(good, "rb").read()
    enc_only = _write(tmp_path / "enc.bin", hp, gf.synthetic_weights(hp, 1), "f16")
    base = open(enc_only, "rb").read()

    def record(name, arr, ftype):
        import struct
        a = np.asarray(arr, dtype=np.float32)
        nm = name.encode()
        t = ftype if a.ndim == 2 else 0
        rec = struct.pack("<3i", a.ndim, len(nm), t) + b"".join(struct.pack("<i", a.shape[a.ndim - 1 - i]) for i in range(a.ndim)) + nm
        return rec + (a.astype(np.float16).tobytes() if t == 1 else a.tobytes())

    def file_with(*recs):
        p = str(tmp_path / f"case{len(os.listdir(tmp_path))}.bin")
        open(p, "wb").write(base + b"".join(recs))
        return p

    full = [record(n, w[n], 1) for n in gf.HEAD_NAMES]
    assert file_with(*full) and open(file_with(*full), "rb").read() == data          # (the records are the writer's)
    for missing in range(4):
        err = _digest_error(file_with(*[r for i, r in enumerate(full) if i != missing]), capfd)
        assert "partial classification head" in err and gf.HEAD_NAMES[missing] in err, err
    err = _digest_error(file_with(record("pooler.dense.weight", np.zeros((H, H + 32)), 1), *full[1:]), capfd)
    assert "pooler.dense.weight" in err and ("wrong shape" in err or "wrong size" in err), err
    err = _digest_error(file_with(full[0], full[1], full[2], record("classifier.bias", np.zeros(4), 1)), capfd)
    assert "classifier.bias" in err and "wrong shape" in err, err
    err = _digest_error(file_with(full[0], full[1], record("classifier.weight", np.zeros((3, H + 32)), 1), full[3]), capfd)
    assert "classifier.weight" in err and "wrong shape" in err, err
    err = _digest_error(file_with(full[0], full[1], record("classifier.weight", np.zeros((9, H)), 1), record("classifier.bias", np.zeros(9), 1)), capfd)
    assert "n_labels = 9 outside 1 .. 8" in err, err
    err = _digest_error(file_with(record("pooler.dense.weigh", w["pooler.dense.weight"], 1)), capfd)
    assert "unknown tensor 'pooler.dense.weigh'" in err, err


@pytest.mark.parametrize("ftype", ["q4_0", "q4_1"])
def test_legacy_q4_file_with_a_head_is_refused(tmp_path, ftype, capfd):
    """Nothing ever wrote a legacy-q4 file with a head: the block-layout detection sums the encoder's set only, so such a file is read
    in the current layout, fails to parse and is refused; the same legacy file without the head still loads."""
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 2, n_labels=1)
    leg = _write(tmp_path / "leg.bin", hp, {n: a for n, a in w.items() if n not in gf.HEAD_NAMES}, ftype, legacy_q4=True)
    assert libbert.model_digest(leg)[1] is True
    bad = _write(tmp_path / "leg_head.bin", hp, w, ftype, legacy_q4=True)
    err = _digest_error(bad, capfd)
    assert "bert_hip_test_model_digest:" in err


@pytest.mark.parametrize("qtype", [2, 3])
def test_quantize_tool_carries_the_head_through(tmp_path, qtype):
    """bert-quantize knows the head by the format's own rule (2-D "*weight" tensors are quantized, everything else copied): its output
    is byte for byte the file ggml_file writes in that type from the same f16 values, and the product's parser accepts it."""
    from conftest import ROOT
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "tools"], check=True, stdout=subprocess.DEVNULL)
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 4, n_labels=3)
    src, out = _write(tmp_path / "f16.bin", hp, w, "f16"), str(tmp_path / "q.bin")
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-quantize"), src, out, str(qtype)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = gf.read_model(out), gf.read_model(_write(tmp_path / "py.bin", hp, w, gf.FTYPE_NAMES[qtype]))
    assert list(got.raw) == list(want.raw) and list(got.raw)[-4:] == gf.HEAD_NAMES
    for n in gf.HEAD_NAMES:
        assert got.raw[n][:2] == want.raw[n][:2] and bytes(got.raw[n][2]) == bytes(want.raw[n][2]), n
    assert libbert.model_digest(out)[0] == 5 + 16 * hp.n_layer + 4


# ------------------------------------------------------------------------------------------------
# tokenize_pair
# ------------------------------------------------------------------------------------------------
def _expected_pair(m, a, b, n):
    A, B = m.tokenize_long(a), m.tokenize_long(b)[1:]
    if len(A) + len(B) <= n:
        return A + B, len(A)
    na = min(len(A), n // 2)
    nb = min(len(B), n - na)
    return A[:na - 1] + [102] + B[:nb - 1] + [102], na


@pytest.mark.parametrize("n_max", [12, 64])
def test_tokenize_pair(sparse_vocab_model, tok_golden, n_max):
    m = libbert.BertModel(sparse_vocab_model, tokenizer_only=True)
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()][:40]
    assert len(words) >= 8
    short, long_ = " ".join(words[:3]), " ".join(words * 4)
    assert len(m.tokenize_long(short)) <= 6 and len(m.tokenize_long(long_)) > 64
    for a, b in [(short, short), (long_, short), (short, long_), (long_, long_), (short, ""), ("", short), (long_, "")]:
        ids, fl = m.tokenize_pair(a, b, n_max)
        want, want_fl = _expected_pair(m, a, b, n_max)
        assert (ids, fl) == (want, want_fl), (a[:20], b[:20])
        assert len(ids) <= n_max and ids[0] == 101 and ids[fl - 1] == 102 and ids[-1] == 102 and ids.count(101) == 1
        if len(m.tokenize_long(a)) + len(m.tokenize_long(b)) - 1 <= n_max:
            assert ids == m.tokenize(a) + m.tokenize(b)[1:] and fl == len(m.tokenize(a))
    ids, fl = m.tokenize_pair(short, "", n_max)
    assert ids == m.tokenize(short) + [102]
    assert m.n_labels == 0
    m.close()


# ------------------------------------------------------------------------------------------------
# semantics and bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_labels", [1, 3])
def test_float64_model_matches_huggingface(tmp_path, n_labels):
    """cross_encoder_reference.Model against transformers.BertForSequenceClassification(...).double() (gelu_new, eps 1e-5, no dropout)
    on the tiny dims with token types: logits within 1e-9."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hf_cross_encoder_reference.py")
    r = subprocess.run([sys.executable, script, "tiny", str(n_labels), str(tmp_path)], capture_output=True, text=True, timeout=600)
    if r.returncode == 77:
        pytest.skip("torch / transformers not importable")
    assert r.returncode == 0, r.stderr[-2000:]
    ref = np.load(str(tmp_path / f"hf_ce_{n_labels}.npz"))
    model = cer.Model(str(tmp_path / f"hf_ce_tiny_{n_labels}.bin"))
    assert model.n_labels == n_labels and int(ref["n"]) == 5
    for i in range(int(ref["n"])):
        got = model.logits(ref[f"ids{i}"], int(ref[f"first{i}"]))
        assert got.shape == (n_labels,) and np.abs(got - ref[f"want{i}"]).max() <= 1e-9, (i, got, ref[f"want{i}"])
    # types reach the reference: another first_len, another logit
    assert np.abs(model.logits(ref["ids1"], 9) - model.logits(ref["ids1"], 20)).max() > 1e-6


@pytest.mark.parametrize("H", [24, 64, 384])
@pytest.mark.parametrize("scale", [0.01, 1.0, 30.0])
def test_head_bound_holds_for_the_f32_emulation(H, scale):
    """The f32 NumPy emulation of the matrix-core head (f16 operands, f32 sums in the kernel's order) lies within head_bound of float64,
    logits and sigmoid, for rows from the linear range of tanh to saturation."""
    rng = np.random.default_rng(H)
    B, NL = 5, 3
    rows = (rng.normal(0, scale, (B, H))).astype(np.float32)
    Wp = rng.normal(0, 1 / np.sqrt(H), (H, H)).astype(np.float32)
    bp, Wc, bc = rng.normal(0, 0.1, H).astype(np.float32), rng.normal(0, 1 / np.sqrt(H), (NL, H)).astype(np.float32), rng.normal(0, 0.1, NL).astype(np.float32)
    for sig in (False, True):
        got = cer.head_emulated_f32(rows, Wp, bp, Wc, bc, sig).astype(np.float64)
        want = cer.head(rows, Wp, bp, Wc, bc, sig)
        bound = cer.head_bound(rows, 0.0, Wp, bp, Wc, bc, True, sig)
        assert (np.abs(got - want) <= bound).all(), (H, scale, sig, float((np.abs(got - want) / bound).max()))
        if scale <= 1.0:
            assert bound.max() < 0.2, float(bound.max())     # (worst-case sums of magnitudes, but still a bound that says something)
