"""Test infrastructure of the cross-encoder tests (test_cross_encoder_host.py, test_gpu_cross_encoder.py): a float64 NumPy forward of the
whole model from a ggml_file.read_model file — typed embedding, encoder layers, [CLS] row, classification head — on the dequantised
weights; the derived error bound of the head; and an f32 NumPy emulation of the head in the matrix-core kernel's order.

The model (reference bert.cpp:784-913 plus HuggingFace BertForSequenceClassification's pooler and classifier): x = LayerNorm(word[id] +
type[t] + pos[p]); per layer x = LN(x + attn(x) Wo^T + bo), x = LN(x + gelu_tanh(x W1^T + b1) W2^T + b2), eps 1e-5, softmax(q k^T /
sqrt(d_head)) without a mask (a sentence is evaluated alone); logits = Wc tanh(Wp x[0] + bp) + bc."""
import dataclasses

import numpy as np

from bert_cpp_amd import ggml_file as gf
from f32_reference import TANHF_ULP
from layer_reference import U16, U32, f8, gelu, layernorm


class Model:
    """The dequantised tensors of a model file as float64."""

    def __init__(self, path):
        self.mf = gf.read_model(path)
        self.hp = self.mf.hp
        self.t = {n: f8(self.mf.dequantized(n)) for n in self.mf.raw}
        self.n_labels = self.t["classifier.weight"].shape[0] if "classifier.weight" in self.t else 0

    def embed(self, ids, first_len=None):
        """LayerNorm of word + type + position; first_len leading tokens take type row 0, the rest row 1 (None: all row 0)."""
        ids = np.asarray(ids)
        n = len(ids)
        tt = np.zeros(n, dtype=np.int64) if first_len is None else (np.arange(n) >= first_len).astype(np.int64)
        pre = self.t["embeddings.word_embeddings.weight"][ids] + self.t["embeddings.token_type_embeddings.weight"][tt] + \
            self.t["embeddings.position_embeddings.weight"][np.arange(n)]
        return layernorm(pre, self.t["embeddings.LayerNorm.weight"], self.t["embeddings.LayerNorm.bias"])

    def layer(self, x, i):
        t, p = self.t, f"encoder.layer.{i}."
        nh, dh = self.hp.n_head, self.hp.n_embd // self.hp.n_head
        q, k, v = (x @ t[p + f"attention.self.{w}.weight"].T + t[p + f"attention.self.{w}.bias"] for w in ("query", "key", "value"))
        ctx = np.empty_like(x)
        for h in range(nh):
            s = slice(h * dh, (h + 1) * dh)
            a = q[:, s] @ k[:, s].T / np.sqrt(dh)
            a = np.exp(a - a.max(axis=1, keepdims=True))
            ctx[:, s] = (a / a.sum(axis=1, keepdims=True)) @ v[:, s]
        y = layernorm(x + ctx @ t[p + "attention.output.dense.weight"].T + t[p + "attention.output.dense.bias"],
                      t[p + "attention.output.LayerNorm.weight"], t[p + "attention.output.LayerNorm.bias"])
        ff = gelu(y @ t[p + "intermediate.dense.weight"].T + t[p + "intermediate.dense.bias"])
        return layernorm(y + ff @ t[p + "output.dense.weight"].T + t[p + "output.dense.bias"], t[p + "output.LayerNorm.weight"],
                         t[p + "output.LayerNorm.bias"])

    def states(self, ids, first_len=None):
        """final token states [n, H]"""
        x = self.embed(ids, first_len)
        for i in range(self.hp.n_layer):
            x = self.layer(x, i)
        return x

    def cls_row(self, ids, first_len=None):
        return self.states(ids, first_len)[0]

    def head_weights(self):
        t = self.t
        return t["pooler.dense.weight"], t["pooler.dense.bias"], t["classifier.weight"], t["classifier.bias"]

    def logits(self, ids, first_len=None):
        return head(self.cls_row(ids, first_len)[None], *self.head_weights())[0]


def head(rows, Wp, bp, Wc, bc, sigmoid=False):
    """float64: rows [B, H] -> [B, n_labels]"""
    z = np.tanh(f8(rows) @ f8(Wp).T + f8(bp)) @ f8(Wc).T + f8(bc)
    return 1.0 / (1.0 + np.exp(-z)) if sigmoid else z


def head_bound(rows, drows, Wp, bp, Wc, bc, mfma=True, sigmoid=False):
    """Per-element bound [B, n_labels] on |device head - head()| for rows that are off by at most drows (a scalar or [B, H]) from the rows
    head() is given.  Wp: the values the DEVICE holds before its own rounding (the dequantised file values).  First order, term by term:
      pooler pre-activation a = <row, Wp[f]> + bp[f], S = sum |row| |Wp[f]| + |bp[f]|:
        mfma: the row and Wp rounded to f16, 2^-11 each (q4_1 values are rounded once from a double: 2^-24 more) -> (2 U16 + U32) sum |row| |Wp[f]|;
        f32 accumulation of H + 1 terms in any order, (H + 4) 2^-24 S, times the repository's factor 4 for the matrix cores' internal
        rounding (layer_reference.matmul_bound); the plain form: the same sum without the factor and without the f16 roundings;
        the input perturbation: drows |Wp[f]| summed;
      p = tanh(a): d p <= (1 - tanh^2(a)) da to first order — and never more than da, which also covers the saturated range where the
        first-order factor vanishes but a large da could leave it; plus TANHF_ULP ulp of f32 at p;
      logit = sum_f p Wc[l][f] + bc[l]: dp |Wc| summed, plus the f32 sum of H + 1 terms (fmaf chains, a butterfly, a tree: any order),
        (H + 4) 2^-24 (sum |p| |Wc| + |bc|);
      sigmoid: slope <= 1 / 4, plus 4 ulp of f32 at the result for expf and the division."""
    rows, Wp, bp, Wc, bc = (f8(a) for a in (rows, Wp, bp, Wc, bc))
    H = rows.shape[1]
    drows = np.broadcast_to(f8(drows), rows.shape)
    aW = np.abs(Wp)
    P = np.abs(rows) @ aW.T                                   # [B, H]: sum |row| |Wp[f]|
    S = P + np.abs(bp)
    da = (4 if mfma else 1) * (H + 4) * U32 * S + ((2 * U16 + U32) * P if mfma else 0.0) + drows @ aW.T
    a = rows @ Wp.T + bp
    p = np.tanh(a)
    # (second order of tanh: |tanh''| <= 0.77; da^2 covers it)
    dp = np.minimum((1 - p * p) * da + da * da, da) + TANHF_ULP * U32 * 2 * np.abs(p) + 2.0 ** -149
    aC = np.abs(Wc)
    dz = dp @ aC.T + (H + 4) * U32 * (np.abs(p) @ aC.T + np.abs(bc))      # [B, n_labels]
    if not sigmoid:
        return dz
    z = p @ Wc.T + bc
    s = 1.0 / (1.0 + np.exp(-z))
    return 0.25 * dz + 4 * U32 * 2 * s + 2.0 ** -149


def head_emulated_f32(rows, Wp, bp, Wc, bc, sigmoid=False):
    """The matrix-core kernel's arithmetic in f32 NumPy, in its order: the rows and Wp rounded to f16, an f32 inner product (the matrix
    cores' internal order is not documented: k ascending here), + bp, tanh in f32; per label, per block of 32 features, per lane half h a
    chain over r = 0 .. 15 of feature (r & 3) + 8 (r >> 2) + 4 h from +0, the halves added, the blocks added in ascending order per wave
    (blocks w, w + 4, ...), the waves as (0 + 1) + (2 + 3), bc last."""
    f = np.float32
    r16 = np.asarray(rows, dtype=f).astype(np.float16).astype(f)
    w16 = np.asarray(Wp, dtype=f).astype(np.float16).astype(f)
    bp, Wc, bc = (np.asarray(a, dtype=f) for a in (bp, Wc, bc))
    B, H = r16.shape
    NL = Wc.shape[0]
    acc = np.zeros((B, H), dtype=f)
    for k in range(H):
        acc = acc + r16[:, k:k + 1] * w16[None, :, k]
    p = np.tanh((acc + bp).astype(f)).astype(f)
    out = np.zeros((B, NL), dtype=f)
    for lab in range(NL):
        wave = [np.zeros(B, dtype=f) for _ in range(4)]
        for blk in range((H + 31) // 32):
            half = []
            for h in range(2):
                s = np.zeros(B, dtype=f)
                for r in range(16):
                    ft = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * h
                    if ft < H:
                        s = (p[:, ft] * Wc[lab, ft] + s).astype(f)
                half.append(s)
            wave[blk % 4] = (wave[blk % 4] + (half[0] + half[1]).astype(f)).astype(f)
        out[:, lab] = (((wave[0] + wave[1]).astype(f) + (wave[2] + wave[3]).astype(f)).astype(f) + bc[lab]).astype(f)
    if sigmoid:
        out = (f(1) / (f(1) + np.exp(-out).astype(f))).astype(f)
    return out


def pair_ids(rng, n_vocab, total, first_len):
    """a sentence of `total` ids: [CLS] .. [SEP] over first_len places, the rest closed by a second [SEP] (first_len <= total)"""
    lo = 1000 if n_vocab > 2000 else min(104, n_vocab - 1)
    ids = rng.integers(lo, n_vocab, size=total).astype(np.int32)
    cls, sep = (101, 102) if n_vocab > 102 else (1, 2)
    ids[0] = cls
    if 1 <= first_len <= total:
        ids[first_len - 1] = sep
    ids[-1] = sep
    return ids


# ------------------------------------------------------------------------------------------------
# the end-to-end batches (test_gpu_cross_encoder.py; tools/cross_encoder_parity.py measures the parent commit on the same ids)
# ------------------------------------------------------------------------------------------------
# the tiny dims with a position table of 256 rows: the pair lengths go up to 200
DIMS = {"tiny": dataclasses.replace(gf.MODEL_DIMS["tiny"], n_max_tokens=256), "tiny-h128": dataclasses.replace(gf.MODEL_DIMS["tiny-h128"], n_max_tokens=256),
        "minilm-l6": gf.MODEL_DIMS["minilm-l6"]}
E2E_MODELS = [("tiny", "f32"), ("tiny", "f16"), ("tiny", "q4_0"), ("tiny-h128", "f16"), ("minilm-l6", "f16"), ("minilm-l6", "q4_1")]
E2E_SEED = 5
PAIRS = [(total, first) for total in (3, 37, 128, 200) for first in (2, 9, 64, 100) if first <= total]
# small batches; one with sentences beyond a window of 128 tokens; 16 x 128 tokens (full windows: the one-launch route from the lane-order embedding)
BATCHES = {"short": [p for p in PAIRS if p[0] <= 128], "long": [p for p in PAIRS if p[0] > 128] + [(3, 2), (37, 9)],
           "full": [(128, f) for f in (2, 9, 64, 100)] * 4}


def batch(rng, hp, pairs):
    """(tokens, cu_seqlens, first_len, sentences) of (total, first_len) pairs"""
    sents = [pair_ids(rng, hp.n_vocab, total, first) for total, first in pairs]
    cu = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int32)
    return np.concatenate(sents).astype(np.int32), cu, np.array([f for _, f in pairs], dtype=np.int32), sents


def e2e_batches(dims):
    """name -> batch(): the batches of the end-to-end test and of the parent's measurement, the same ids"""
    return {name: batch(np.random.default_rng(100 + i), DIMS[dims], pairs) for i, (name, pairs) in enumerate(BATCHES.items())}
