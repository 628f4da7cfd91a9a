"""CPU-side tests of the learned sparse embeddings (bert_hip.h "learned sparse embeddings"): the optional MLM head in the model file, the
float64 reference model against HuggingFace, the weights' error bound against an f32 emulation, the top-k rule, the sparsity of the
end-to-end batches, the new symbols and the launch geometry of the vocabulary kernel."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert as libbert

import sparse_reference as sr

FTYPES = ["f32", "f16", "q4_0", "q4_1"]
NEW_SYMBOLS = ["bert_hip_has_mlm_head", "bert_hip_sparse_packed", "bert_hip_sparse_packed_device", "bert_hip_sparse_topk_packed",
               "bert_hip_sparse_topk_packed_device", "bert_hip_encode_sparse_batch"]
NEW_TEST_SYMBOLS = ["bert_hip_test_sparse_vocab", "bert_hip_test_sparse_topk", "bert_hip_test_sparse_vocab_geometry", "bert_hip_test_attention_grid"]


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
@pytest.mark.parametrize("n_labels", [0, 3])
def test_mlm_head_file_round_trips_and_loads(tmp_path, ftype, n_labels):
    """A file with the MLM head reads back through ggml_file with every tensor, the head's five behind the encoder's and the
    classification head's; the product's parser accepts it; the same seed gives the same encoder and classification head without it."""
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 3, n_labels=n_labels, mlm_head=True)
    w0 = gf.synthetic_weights(hp, 3, n_labels=n_labels)
    assert all(np.array_equal(w[n], w0[n]) for n in w0) and set(w) - set(w0) == set(gf.MLM_HEAD_NAMES)
    assert {n: a.shape for n, a in w.items() if n in gf.MLM_HEAD_NAMES} == gf.mlm_head_shapes(hp)
    assert (w["cls.predictions.bias"] < 0).mean() > 0.9
    with_head, without = _write(tmp_path / "h.bin", hp, w, ftype), _write(tmp_path / "n.bin", hp, w0, ftype)
    mf = gf.read_model(with_head)
    n_other = 5 + 16 * hp.n_layer + (4 if n_labels else 0)
    assert list(mf.raw)[-5:] == gf.MLM_HEAD_NAMES and len(mf.raw) == n_other + 5
    if n_labels:
        assert list(mf.raw)[-9:-5] == gf.HEAD_NAMES
    ft = gf.FTYPE_BY_NAME[ftype]
    assert mf.raw[gf.MLM_HEAD_NAMES[0]][:2] == (ft, (hp.n_embd, hp.n_embd)) and mf.raw[gf.MLM_HEAD_NAMES[4]][:2] == (0, (hp.n_vocab,))
    for n in gf.MLM_HEAD_NAMES[1:4]:
        assert mf.raw[n][:2] == (0, (hp.n_embd,))
    tol = {"f32": 0, "f16": 1e-3, "q4_0": 0.2, "q4_1": 0.2}[ftype]
    for n in gf.MLM_HEAD_NAMES:
        assert np.abs(mf.dequantized(n) - w[n]).max() <= tol * max(1.0, np.abs(w[n]).max())
    n1, leg1, d1 = libbert.model_digest(with_head)
    n0, leg0, d0 = libbert.model_digest(without)
    assert (n1, leg1) == (n_other + 5, False) and (n0, leg0) == (n_other, False) and d0 != d1


def test_mlm_head_file_refusals(tmp_path, capfd):
    """A partial MLM head, a wrong shape and another unknown name are refused, each with its message."""
    hp = gf.MODEL_DIMS["tiny"]
    H, V = hp.n_embd, hp.n_vocab
    w = gf.synthetic_weights(hp, 1, mlm_head=True)
    good = _write(tmp_path / "good.bin", hp, w, "f16")
    base = open(_write(tmp_path / "enc.bin", hp, gf.synthetic_weights(hp, 1), "f16"), "rb").read()

    def record(name, arr, ftype):
        a = np.asarray(arr, dtype=np.float32)
        nm = name.encode()
        t = ftype if a.ndim == 2 else 0
        rec = struct.pack("<3i", a.ndim, len(nm), t) + b"".join(struct.pack("<i", a.shape[a.ndim - 1 - i]) for i in range(a.ndim)) + nm
        return rec + (a.astype(np.float16).tobytes() if t == 1 else a.tobytes())

    def file_with(*recs):
        p = str(tmp_path / f"case{len(os.listdir(tmp_path))}.bin")
        open(p, "wb").write(base + b"".join(recs))
        return p

    full = [record(n, w[n], 1) for n in gf.MLM_HEAD_NAMES]
    assert open(file_with(*full), "rb").read() == open(good, "rb").read()          # (the records are the writer's)
    for missing in range(5):
        err = _digest_error(file_with(*[r for i, r in enumerate(full) if i != missing]), capfd)
        assert "partial MLM head" in err and gf.MLM_HEAD_NAMES[missing] in err, err
    err = _digest_error(file_with(record(gf.MLM_HEAD_NAMES[0], np.zeros((H, H + 32)), 1), *full[1:]), capfd)
    assert gf.MLM_HEAD_NAMES[0] in err and ("wrong shape" in err or "wrong size" in err), err
    err = _digest_error(file_with(*full[:4], record(gf.MLM_HEAD_NAMES[4], np.zeros(V + 1), 1)), capfd)
    assert gf.MLM_HEAD_NAMES[4] in err and ("wrong shape" in err or "wrong size" in err), err
    err = _digest_error(file_with(full[0], record(gf.MLM_HEAD_NAMES[1], np.zeros(H - 1), 1), *full[2:]), capfd)
    assert gf.MLM_HEAD_NAMES[1] in err and ("wrong shape" in err or "wrong size" in err), err
    for name in ("cls.predictions.decoder.weight", "cls.predictions.transform.dense.weigh"):
        err = _digest_error(file_with(record(name, w[gf.MLM_HEAD_NAMES[0]], 1)), capfd)
        assert f"unknown tensor '{name}'" in err, err


@pytest.mark.parametrize("qtype", [2, 3])
def test_quantize_tool_carries_the_mlm_head_through(tmp_path, qtype):
    """bert-quantize knows the head by the format's own rule (2-D "*weight" tensors are quantized, everything else copied): its output
    is byte for byte the file ggml_file writes in that type from the same f16 values, and the product's parser accepts it."""
    from conftest import ROOT
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "tools"], check=True, stdout=subprocess.DEVNULL)
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 4, n_labels=2, mlm_head=True)
    src, out = _write(tmp_path / "f16.bin", hp, w, "f16"), str(tmp_path / "q.bin")
    r = subprocess.run([os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-quantize"), src, out, str(qtype)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, want = gf.read_model(out), gf.read_model(_write(tmp_path / "py.bin", hp, w, gf.FTYPE_NAMES[qtype]))
    assert list(got.raw) == list(want.raw) and list(got.raw)[-5:] == gf.MLM_HEAD_NAMES
    for n in gf.MLM_HEAD_NAMES:
        assert got.raw[n][:2] == want.raw[n][:2] and bytes(got.raw[n][2]) == bytes(want.raw[n][2]), n
    assert libbert.model_digest(out)[0] == 5 + 16 * hp.n_layer + 4 + 5


def test_new_symbols_are_declared_and_listed():
    """The new entry points are in bert_hip.h and pybert's list, the hooks in bert_hip_test.h and its list — and not in bert_hip.h."""
    from conftest import ROOT
    pub = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    hooks = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"BERT_API int32_t " + s + r"\(", pub) and s in libbert.BERT_HIP_H_SYMBOLS, s
    for s in NEW_TEST_SYMBOLS:
        assert re.search(r"BERT_API int32_t " + s + r"\(", hooks) and s in libbert.BERT_HIP_TEST_H_SYMBOLS and s not in pub, s


# ------------------------------------------------------------------------------------------------
# semantics, bound, top-k
# ------------------------------------------------------------------------------------------------
def test_float64_model_matches_huggingface(tmp_path):
    """sparse_reference.Model against transformers.BertForMaskedLM(...).double() (gelu_new, eps 1e-5, tied decoder) on the tiny dims:
    logits within 1e-9; the weights are the max over the tokens of log1p(relu(logit))."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hf_mlm_reference.py")
    r = subprocess.run([sys.executable, script, "tiny", str(tmp_path)], capture_output=True, text=True, timeout=600)
    if r.returncode == 77:
        pytest.skip("torch / transformers not importable")
    assert r.returncode == 0, r.stderr[-2000:]
    ref = np.load(str(tmp_path / "hf_mlm.npz"))
    model = sr.Model(str(tmp_path / "hf_mlm_tiny.bin"))
    assert model.mlm_head and int(ref["n"]) == 4
    for i in range(int(ref["n"])):
        ids, want = ref[f"ids{i}"], ref[f"want{i}"]
        got = model.logits(ids)
        assert got.shape == want.shape == (len(ids), model.hp.n_vocab) and np.abs(got - want).max() <= 1e-9, (i, float(np.abs(got - want).max()))
        w = model.weights(ids)
        assert np.abs(w - np.log1p(np.maximum(want, 0)).max(axis=0)).max() <= 1e-9
        assert np.abs(w - sr.sparse(model.transform(model.states(ids)), model.mlm_weights()[4], model.mlm_weights()[5], [len(ids)])[0]).max() <= 1e-12


@pytest.mark.parametrize("H", [8, 24, 26, 64, 384])
@pytest.mark.parametrize("scale", [0.05, 1.0])
def test_sparse_bound_holds_for_the_f32_emulation(H, scale):
    """The f32 NumPy emulation of both forms lies within sparse_bound of float64; the bound says something; non-positive z gives +0."""
    rng = np.random.default_rng(H)
    lens, V = [1, 4, 37], 70
    t = rng.normal(0, 1, (sum(lens), H)).astype(np.float32)
    E = rng.normal(0, scale, (V, H)).astype(np.float32)
    bias = rng.normal(-scale * np.sqrt(H), scale * np.sqrt(H), V).astype(np.float32)
    for mfma in (True, False):
        if mfma and H % 8:
            continue
        got = sr.sparse_emulated_f32(t, E, bias, lens, mfma)
        want = sr.sparse(t, E, bias, lens)
        bound = sr.sparse_bound(t, 0.0, E, bias, lens, mfma)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (H, scale, mfma, float((err / bound).max()))
        assert bound.max() < (0.05 if mfma else 1e-3) * scale * H, float(bound.max())
        assert ((got == 0) == (want == 0)).mean() > 0.97 and 0.1 < (want == 0).mean() < 0.9
        assert not np.signbit(got[got == 0]).any()


def test_topk_rule():
    w = np.array([[0.0, 3.0, 1.0, 3.0, -2.0, 0.5], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]], dtype=np.float32)
    ids, wt = sr.topk(w, 4)
    assert ids.tolist() == [[1, 3, 2, 5], [-1, -1, -1, -1], [0, 1, 2, 3]]
    assert wt.tolist() == [[3, 3, 1, 0.5], [0, 0, 0, 0], [1, 1, 1, 1]]
    ids, wt = sr.topk(w, 1)
    assert ids.tolist() == [[1], [-1], [0]]


# ------------------------------------------------------------------------------------------------
# the end-to-end batches are sparse
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ftype", sr.E2E_MODELS)
def test_end_to_end_batches_are_sparse(tmp_path, dims, ftype):
    """On every end-to-end batch of test_gpu_sparse.py between 20 % and 80 % of the float64 model's weights are exactly zero: the relu edge
    and the -1 padding of top-k are exercised.  (The synthetic cls.predictions.bias is drawn for this.)"""
    path = _write(tmp_path / "m.bin", sr.DIMS[dims], sr.model_weights(dims), ftype)
    ref = sr.Model(path)
    for name, (_, _, sents) in sr.e2e_batches(dims).items():
        w = np.stack([ref.weights(s) for s in sents])
        zero = float((w == 0).mean())
        print(f"{dims} {ftype} {name}: {zero:.3f} of the weights are zero; per sentence {[round(float((r == 0).mean()), 2) for r in w]}")
        assert 0.2 <= zero <= 0.8, (dims, ftype, name, zero)
        assert (w >= 0).all() and np.isfinite(w).all()


# ------------------------------------------------------------------------------------------------
# the launch geometry of the matrix-core vocabulary kernel (kernels.h sparse_vocab_geometry; no GPU)
# ------------------------------------------------------------------------------------------------
def _geometry_rule(H, V, T, ns, max_len):
    """launch_sparse_vocab's grid arithmetic as the kernel's header states it, in Python integers; None where the launcher refuses"""
    if min(H, V, T, ns, max_len) <= 0 or H < 8 or H % 8 or H > 1024:
        return None
    tile = 128 if H <= 624 else 64
    nblk = -(-V // 32)
    n_tiles = -(-min(T, ns * max_len) // tile)
    slabs_wanted = max(1, -(-1024 // n_tiles))
    slab_blocks = min(64, max(8, -(--(-nblk // slabs_wanted) // 8) * 8))
    n_slabs = -(-nblk // slab_blocks)
    if n_slabs > 65535:
        return None
    return dict(tile=tile, n_tiles=n_tiles, slab_blocks=slab_blocks, n_slabs=n_slabs)


# (H, V, T, ns, max_len) -> geometry: the shapes of test_gpu_launch_geometry.py, of test_gpu_sparse.py (all 8-block slabs) and of
# profiles/sparse_rate.txt
GEOMETRY_TABLE = [
    ((64, 16421, 2048, 40, 128), dict(tile=128, n_tiles=16, slab_blocks=16, n_slabs=33)),
    ((640, 16421, 1024, 20, 128), dict(tile=64, n_tiles=16, slab_blocks=16, n_slabs=33)),
    ((64, 20001, 4096, 80, 128), dict(tile=128, n_tiles=32, slab_blocks=24, n_slabs=27)),
    ((64, 28737, 8192, 150, 128), dict(tile=128, n_tiles=64, slab_blocks=64, n_slabs=15)),
    ((384, 30522, 32768, 256, 128), dict(tile=128, n_tiles=256, slab_blocks=64, n_slabs=15)),
    ((384, 30522, 8192, 64, 128), dict(tile=128, n_tiles=64, slab_blocks=64, n_slabs=15)),
    ((384, 30522, 333, 3, 200), dict(tile=128, n_tiles=3, slab_blocks=8, n_slabs=120)),
    ((1024, 1000, 513, 1, 513), dict(tile=64, n_tiles=9, slab_blocks=8, n_slabs=4)),
    ((8, 1, 1, 1, 1), dict(tile=128, n_tiles=1, slab_blocks=8, n_slabs=1)),
    ((624, 250, 128, 1, 128), dict(tile=128, n_tiles=1, slab_blocks=8, n_slabs=1)),
    ((632, 250, 128, 1, 128), dict(tile=64, n_tiles=2, slab_blocks=8, n_slabs=1)),
    ((64, 28737, 8192, 9, 128), dict(tile=128, n_tiles=9, slab_blocks=8, n_slabs=113)),        # (a piece of nine sentences)
    ((64, 28737, 8192, 10, 128), dict(tile=128, n_tiles=10, slab_blocks=16, n_slabs=57)),
]


@pytest.mark.parametrize("shape,want", GEOMETRY_TABLE, ids=[str(s) for s, _ in GEOMETRY_TABLE])
def test_vocabulary_geometry_table(shape, want):
    """The geometry hook on written-out shapes (the values worked by hand from the rule in sparse_vocab.hip), and the Python rule agrees."""
    assert libbert.test_sparse_vocab_geometry(*shape) == want
    assert _geometry_rule(*shape) == want


def test_vocabulary_geometry_invariants():
    """Over a sweep of (H, V, T, ns, max_len), V up to 2^24 - 1: slab_blocks is a multiple of 8 in 8 .. 64; the slabs cover the vocabulary
    blocks and the last one is not empty; the tiles cover the served tokens; the call is refused exactly where the launcher refuses; every
    value is the rule's."""
    Hs = [0, 4, 8, 20, 24, 64, 384, 624, 632, 640, 768, 1024, 1032]
    Vs = [0, 1, 31, 32, 33, 250, 257, 8192, 16421, 20001, 28737, 30522, 250002, (1 << 24) - 1]
    Ts = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 2048, 8192, 32768, 262144, (1 << 31) - 1]
    nss = [0, 1, 3, 64, 300, 65535, 1 << 24]
    max_lens = [0, 1, 33, 128, 512, 1 << 20]
    seen, n = set(), 0
    for H in Hs:
        for V in Vs:
            for T in Ts:
                for ns in nss:
                    for max_len in max_lens:
                        got = libbert.test_sparse_vocab_geometry(H, V, T, ns, max_len)
                        refused = min(V, T, ns, max_len) <= 0 or H < 8 or H % 8 != 0 or H > 1024
                        assert (got is None) == refused, (H, V, T, ns, max_len, got)
                        assert got == _geometry_rule(H, V, T, ns, max_len), (H, V, T, ns, max_len, got)
                        if got is None:
                            continue
                        n += 1
                        nblk, sb = (V + 31) // 32, got["slab_blocks"]
                        assert sb % 8 == 0 and 8 <= sb <= 64
                        assert got["n_slabs"] * sb >= nblk > (got["n_slabs"] - 1) * sb
                        assert got["tile"] == (128 if H <= 624 else 64)
                        assert got["n_tiles"] * got["tile"] >= min(T, ns * max_len) > (got["n_tiles"] - 1) * got["tile"]
                        seen.add(sb)
    assert {8, 16, 24, 32, 64} <= seen and n > 10000, (sorted(seen), n)
    # the one refusal beyond the arguments: more slabs than a grid dimension holds (never below V = 2^24)
    assert libbert.test_sparse_vocab_geometry(64, 65536 * 64 * 32, 1 << 20, 8192, 128) is None
    assert libbert.test_sparse_vocab_geometry(64, 65535 * 64 * 32, 1 << 20, 8192, 128) == dict(tile=128, n_tiles=8192, slab_blocks=64, n_slabs=65535)
