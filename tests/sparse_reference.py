"""Test infrastructure of the learned-sparse-embedding tests (test_sparse_host.py, test_gpu_sparse.py; tools/sparse_parity.py): a float64
model with the masked-language-model head — cross_encoder_reference.Model plus the transform, the tied projection and the max —, the
derived per-element bound of the weights, an f32 NumPy emulation of the device's arithmetic, the top-k rule, and the end-to-end batches.

w[b][v] = max over the tokens i of sentence b of log1p(relu(<t_i, E_v> + bias[v])), t = LayerNorm(gelu_tanh(x Wt^T + bt)) (eps 1e-5) over
the final states x, E the word-embedding matrix (HuggingFace BertForMaskedLM with the decoder tied, pooled as SPLADE does).  log1p and relu
are monotone, so this equals log1p(relu(max_i <t_i, E_v> + bias[v])): what the device computes."""
import dataclasses

import numpy as np

from bert_cpp_amd import ggml_file as gf
import cross_encoder_reference as cer
import f32_reference as f32r
import layer_reference as lr
from layer_reference import U16, U32, f8, gelu, layernorm

LOG1PF_ULP = 4.0            # log1pf: not measured; twice OpenCL's full-profile requirement of 2 ulp


class Model(cer.Model):
    """cross_encoder_reference.Model with the MLM head."""

    def __init__(self, path):
        super().__init__(path)
        self.mlm_head = gf.MLM_HEAD_NAMES[0] in self.t

    def mlm_weights(self):
        """(Wt, bt, gamma, beta, E, bias)"""
        return tuple(self.t[n] for n in gf.MLM_HEAD_NAMES[:4]) + (self.t["embeddings.word_embeddings.weight"], self.t[gf.MLM_HEAD_NAMES[4]])

    def transform(self, x):
        Wt, bt, g, b, _, _ = self.mlm_weights()
        return layernorm(gelu(f8(x) @ Wt.T + bt), g, b)

    def logits(self, ids, first_len=None):
        """[n, V]: BertForMaskedLM's logits"""
        _, _, _, _, E, bias = self.mlm_weights()
        return self.transform(self.states(ids)) @ E.T + bias

    def weights(self, ids):
        """[V]"""
        return np.log1p(np.maximum(self.logits(ids), 0.0)).max(axis=0)


def _segments(lens):
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [(int(cu[b]), int(cu[b + 1])) for b in range(len(lens))]


def sparse(t, E, bias, lens):
    """float64: t [T, H] transformed token rows of packed sentences, E [V, H], bias [V] -> [B, V]"""
    p = f8(t) @ f8(E).T
    return np.stack([np.log1p(np.maximum(p[a:b].max(axis=0) + f8(bias), 0.0)) for a, b in _segments(lens)])


def sparse_bound(t, dt, E, bias, lens, mfma=True, e_rounded=True):
    """Per-element bound [B, V] on |device weights - sparse()| for rows t that are off by at most dt (a scalar or [T, H]) from the rows the
    DEVICE multiplies before its own rounding.  log1p(relu(.)) is 1-Lipschitz, so this is the bound on z = max_i p[i][v] + bias[v], and
    |max_i a_i - max_i b_i| <= max_i |a_i - b_i|.  Term by term, with P = sum_k |t_k| |E_vk| per (token, v):
      - matrix-core form: t and E rounded to f16, 2^-11 each (E only where the file is not f16: e_rounded; a q4_1 value is rounded once
        from a double, 2^-24 more) -> (2 U16 + U32) P; f32 accumulation of H terms in any order, (H + 4) 2^-24 P, times the repository's
        factor 4 for the matrix cores' internal rounding (layer_reference.matmul_bound);
      - plain form: one f32 fmaf chain per lane and a butterfly, (H + 4) 2^-24 P, no operand rounding, no factor;
      - the rows' own error: dt |E_v| summed;
      - the max is exact; + bias is one f32 add: 2^-24 |z|;
      - log1pf: LOG1PF_ULP ulp of f32 at the result, and the smallest subnormal."""
    t, E, bias = f8(t), f8(E), f8(bias)
    H = t.shape[1]
    dt = np.broadcast_to(f8(dt), t.shape)
    aE = np.abs(E)
    P = np.abs(t) @ aE.T
    dp = ((4 * (H + 4) * U32 + ((2 if e_rounded else 1) * U16 + U32)) if mfma else (H + 4) * U32) * P + dt @ aE.T
    p = t @ E.T
    out = []
    for a, b in _segments(lens):
        z = p[a:b].max(axis=0) + bias
        w = np.log1p(np.maximum(z, 0.0))
        out.append(dp[a:b].max(axis=0) + U32 * np.abs(z) + LOG1PF_ULP * U32 * 2 * w + 2.0 ** -149)
    return np.stack(out)


def transform_bound(x, dx, Wt, bt, g, b, f32_route=False, w_rounded=True):
    """Per-element bound [T, H] on |device t - LayerNorm(gelu(x Wt^T + bt))| BEFORE the vocabulary launch's own rounding, for states x that
    are off by at most dx, to first order:
      - the mat-mul: dx |Wt| summed; the matrix rounded to f16 where the file is not f16 (w_rounded: (U16 + U32) S); the accumulation
        (layer_reference.matmul_bound, or f32_reference.matmul_bound on the f32 route);
      - GELU: layer_reference.gelu_bound (which includes the rounding of the stored value to f16) plus |gelu'| <= 1.13 times the
        pre-activation's error; f32_reference.gelu_bound on the f32 route;
      - LayerNorm: layer_reference.layernorm_input_term for the errors of its input, layernorm_bound for its own statistics and the
        rounding of the stored row (f32_reference.layernorm_bound on the f32 route)."""
    x, Wt, bt, g, b = (f8(a) for a in (x, Wt, bt, g, b))
    dx = np.broadcast_to(f8(dx), x.shape)
    pre = x @ Wt.T + bt
    S = np.abs(x) @ np.abs(Wt).T
    if f32_route:
        dpre = f32r.matmul_bound(x, Wt, bt)[0] + dx @ np.abs(Wt).T
        dv = f32r.gelu_bound(pre, dpre)
    else:
        dpre = lr.matmul_bound(x, Wt, bt, 0.0)[0] + dx @ np.abs(Wt).T + ((U16 + U32) * S if w_rounded else 0.0)
        dv = lr.gelu_bound(pre) + 1.13 * dpre
    v = gelu(pre)
    want = layernorm(v, g, b)
    own = f32r.layernorm_bound(v, g, want) if f32_route else lr.layernorm_bound(v, g, want)
    return lr.layernorm_input_term(v, g, dv) + own


def sparse_emulated_f32(t, E, bias, lens, mfma=True):
    """The device's arithmetic in f32 NumPy: operands rounded to f16 (matrix-core form), an f32 inner product with k ascending (the
    matrix cores' internal order is not documented), the max, one f32 add of the bias, relu, log1p in f32."""
    f = np.float32
    t32, e32 = np.asarray(t, dtype=f), np.asarray(E, dtype=f)
    if mfma:
        t32, e32 = t32.astype(np.float16).astype(f), e32.astype(np.float16).astype(f)
    acc = np.zeros((t32.shape[0], e32.shape[0]), dtype=f)
    for k in range(t32.shape[1]):
        acc = (acc + t32[:, k:k + 1] * e32[None, :, k]).astype(f)
    out = []
    for a, b in _segments(lens):
        z = (acc[a:b].max(axis=0) + np.asarray(bias, dtype=f)).astype(f)
        out.append(np.where(z > 0, np.log1p(np.maximum(z, f(0))), f(0)).astype(f))
    return np.stack(out)


def topk(w, k):
    """The top-k rule on dense rows w [n, V]: per row the k largest positive weights, larger first, equal weights smaller id first;
    unused places id -1, weight +0.  -> (ids int32 [n, k], weights float32 [n, k])"""
    w = np.asarray(w, dtype=np.float32)
    ids = np.full((w.shape[0], k), -1, dtype=np.int32)
    out = np.zeros((w.shape[0], k), dtype=np.float32)
    for r, row in enumerate(w):
        pos = np.flatnonzero(row > 0)
        order = pos[np.lexsort((pos, -row[pos].astype(np.float64)))][:k]
        ids[r, :len(order)] = order
        out[r, :len(order)] = row[order]
    return ids, out


def sentence_ids(rng, n_vocab, n):
    """[CLS] .. [SEP] of n ids (n == 1: [CLS] alone)"""
    lo = 1000 if n_vocab > 2000 else min(104, n_vocab - 1)
    ids = rng.integers(lo, n_vocab, size=n).astype(np.int32)
    cls, sep = (101, 102) if n_vocab > 102 else (1, 2)
    ids[-1] = sep
    ids[0] = cls
    return ids


# ------------------------------------------------------------------------------------------------
# the end-to-end batches (test_gpu_sparse.py; tools/sparse_parity.py measures the parent commit on the same ids)
# ------------------------------------------------------------------------------------------------
# the tiny dims with a position table of 256 rows: the sentences go up to 200 tokens
DIMS = {"tiny": dataclasses.replace(gf.MODEL_DIMS["tiny"], n_max_tokens=256), "tiny-d64": dataclasses.replace(gf.MODEL_DIMS["tiny-d64"], n_max_tokens=256),
        "minilm-l6": gf.MODEL_DIMS["minilm-l6"]}
E2E_MODELS = [("tiny", "f32"), ("tiny", "f16"), ("tiny", "q4_0"), ("tiny-d64", "f16"), ("minilm-l6", "f16")]
E2E_SEED = 5
# short sentences in one tile; sentences beyond a tile of 128 slots and across tile edges; minilm-l6: a handful only (the float64 model
# multiplies every token with 30 522 vocabulary rows)
BATCHES = {"short": [1, 4, 5, 33, 17, 2], "long": [200, 3, 128, 37, 150]}
BATCHES_BIG = {"short": [1, 9, 33], "long": [200, 5, 128]}


def batch(rng, hp, lens):
    """(tokens, cu_seqlens, sentences)"""
    sents = [sentence_ids(rng, hp.n_vocab, n) for n in lens]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return np.concatenate(sents).astype(np.int32), cu, sents


def e2e_batches(dims):
    """name -> batch(): the batches of the end-to-end test and of the parent's measurement, the same ids"""
    table = BATCHES_BIG if dims == "minilm-l6" else BATCHES
    return {name: batch(np.random.default_rng(200 + i), DIMS[dims], lens) for i, (name, lens) in enumerate(table.items())}


def model_weights(dims, mlm_head=True):
    """the synthetic weights of an end-to-end model (the same encoder with and without the head)"""
    return gf.synthetic_weights(DIMS[dims], E2E_SEED, mlm_head=mlm_head)
