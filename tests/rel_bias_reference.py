"""Test infrastructure of the relative position bias tests (test_rel_bias_host.py, test_gpu_rel_bias.py): MPNet's bucket function and the
expanded table restated in NumPy, the float64 attention with the bias and the derived error bounds of the three attention kernels,
and a float64 forward of the whole model from a ggml_file.read_model file.

The definition (HuggingFace MPNetEncoder with 32 buckets, max_distance 128): for head h, query i, key j of a sentence
    score(i, j) = <q_i, k_j> / sqrt(d_head) + W[bucket(j - i)][h],      W = encoder.relative_attention_bias.weight [32][n_head],
    bucket(d): m = |d|, base = 16 if d > 0 else 0; m < 8: base + m; else base + 8 + t, t the largest index with THR[t] <= m,
then softmax over j.  One table for all layers.  The rest of the model is BERT's post-LN encoder (cross_encoder_reference.py) with a zero
token-type table and the position table starting at HuggingFace's row 2."""
import functools

import numpy as np

from bert_cpp_amd import ggml_file as gf
from f32_reference import EXPF_ULP
from layer_reference import U16, U32, f8, gelu, layernorm, native_expf_rel, ulp16

THR = np.array([8, 12, 16, 23, 32, 46, 64, 91])
N_BUCKETS = 32
P_OP = 512                               # the table length of the op-level tests
# the bucket edges, the full one-chunk form, the first length of the persistent form, a ragged second chunk, a full launch
LENS = (1, 2, 8, 9, 12, 13, 91, 92, 127, 128, 129, 256, 257, 512)
W_SIGMA = 2.0                            # one wrong bucket moves a softmax far outside any bound


def bucket(d):
    """MPNet's bucket of the distance d = key - query (any integer array)"""
    d = np.asarray(d, dtype=np.int64)
    m = np.abs(d)
    t = np.searchsorted(THR, m, side="right") - 1           # the largest index with THR[t] <= m (-1 below 8)
    return np.where(d > 0, N_BUCKETS // 2, 0) + np.where(m < 8, m, 8 + t)


def rel_table(W, P):
    """W [32][n_head] -> rel [n_head][2 P - 1], rel[h][d + P - 1] = W[bucket(d)][h]: what the engine expands at load"""
    W = np.asarray(W)
    return np.ascontiguousarray(W[bucket(np.arange(-(P - 1), P))].T)


def bias_matrix(W, h, n):
    """float64 b [n][n], b[i][j] = W[bucket(j - i)][h]"""
    i = np.arange(n)
    return f8(np.asarray(W)[bucket(i[None, :] - i[:, None]), h])


def draw_W(n_head, seed=0, sigma=W_SIGMA):
    return np.random.default_rng(1000 + seed).normal(0.0, sigma, (N_BUCKETS, n_head)).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# attention with the bias: float64 and the kernels' bounds
# ------------------------------------------------------------------------------------------------
def attention(q, k, v, b):
    """softmax(q k^T / sqrt(d) + b) v for one head in float64"""
    q, k, v = f8(q), f8(k), f8(v)
    sc = q @ k.T / np.sqrt(q.shape[1]) + b
    p = np.exp(sc - sc.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True) @ v


def mfma_bound(q, k, v, b):
    """layer_reference.softmax_bound (attention.hip's online softmax; its derivation is not repeated) with the bias b [n][n]:
      - the table entry is b sqrt(d) rounded once to f32: 2^-24 |b| of the score in natural units (0 at d_head 64);
      - the add: the kernel either adds the entry to the finished f32 sum (one rounding of |score|) or starts the matrix cores'
        accumulator from it, and then every one of the sum's roundings is taken on a running value of at most |b| sqrt(d) +
        sum |q k|: softmax_bound's term for the sum, 4 (d + 4) 2^-24 sum |q k| scale, with |b| added to sum |q k| scale.  That admits
        both forms (the first costs 2^-24 (|q . k| scale + |b|), less);
      - everything behind the score — the exp2 argument, the chunk maxima, P, L, the output — is softmax_bound's with score + b in
        place of the score.
    Returns (bound, want)."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    scale = 1 / np.sqrt(d)
    sc = q @ k.T * scale + b
    ds = 4 * (d + 4) * U32 * ((np.abs(q) @ np.abs(k).T) * scale + np.abs(b)) + U32 * np.abs(b)
    mx = sc.max(axis=1, keepdims=True)
    first = sc[:, :128].max(axis=1, keepdims=True)
    n_chunks = (n + 127) // 128
    eps = ds + 2.0 ** -22 * (mx - sc) + U32 * (mx - first) + (n_chunks + 1) * 2.0 ** -22
    p = np.exp(sc - mx)
    L = p.sum(axis=1, keepdims=True)
    w = p / L
    dw = w * eps + np.maximum(U16 * w, 2.0 ** -25 / L) + w * (w * eps).sum(axis=1, keepdims=True)
    want = w @ v
    return dw @ np.abs(v) + 8 * (n + 8) * U32 * (w @ np.abs(v)) + ulp16(want), want


def naive_bound(q, k, v, b):
    """layer_reference.generic_attention_bound (attention_naive_kernel) with the bias: the entry is W's own f32 value, exact; the add
    to the scaled score rounds once, 2^-24 |score + b| (fused with the scaling: less); the rest with score + b in place of the score."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    scale = 1 / np.sqrt(d)
    sc = q @ k.T * scale + b
    mx = sc.max(axis=1, keepdims=True)
    eps = (d + 3) * U32 * (np.abs(q) @ np.abs(k).T) * scale + U32 * np.abs(sc) + U32 * (mx - sc) + native_expf_rel(sc - mx)
    p = np.exp(sc - mx)
    L = p.sum(axis=1, keepdims=True)
    w = p / L
    dw = w * eps + 2.0 ** -126 / L
    dw = dw + w * dw.sum(axis=1, keepdims=True)
    want = w @ v
    return dw @ np.abs(v) + (3 * n + 2) * U32 * (w @ np.abs(v)) + ulp16(want), want


def f32_bound(q, k, v, b):
    """f32_reference.softmax_bound (f32_attention_kernel) with the bias, extended as naive_bound extends its own: + 2^-24 |score + b|."""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape
    scale = 1 / np.sqrt(d)
    sc = q @ k.T * scale + b
    mx = sc.max(axis=1, keepdims=True)
    eps = (d + 3) * U32 * (np.abs(q) @ np.abs(k).T) * scale + U32 * np.abs(sc) + U32 * (mx - sc) + 2 * EXPF_ULP * U32
    p = np.exp(sc - mx)
    w = p / p.sum(axis=1, keepdims=True)
    dw = w * eps + w * (w * eps).sum(axis=1, keepdims=True)
    return dw @ np.abs(v) + (2 * n + 2) * U32 * (w @ np.abs(v)), w @ v


BOUNDS = {"mfma": mfma_bound, "naive": naive_bound, "f32": f32_bound}


def attention_packed(qkv, lens, n_head, d_head, W, kind):
    """qkv [T][3H] of packed sentences, W [32][n_head] (None: no bias) -> (float64 context rows [T][H], the bounds of kernel `kind`)"""
    H = n_head * d_head
    want, bnd = np.zeros((len(qkv), H)), np.zeros((len(qkv), H))
    t0 = 0
    for n in lens:
        for h in range(n_head):
            sl = slice(h * d_head, (h + 1) * d_head)
            q, k, v = (qkv[t0:t0 + n, i * H:(i + 1) * H][:, sl] for i in range(3))
            b = bias_matrix(W, h, n) if W is not None else np.zeros((n, n))
            bnd[t0:t0 + n, sl], want[t0:t0 + n, sl] = BOUNDS[kind](q, k, v, b)
        t0 += n
    return want, bnd


@functools.lru_cache(maxsize=None)
def op_inputs(lens, n_head, d_head):
    """qkv [T][3H] as f16 for sentences of `lens` (a tuple): Q a little wide, so that the softmax is neither flat nor one-hot.  Read-only."""
    rng = np.random.default_rng(sum(lens) * 131 + n_head * 17 + d_head)
    H = n_head * d_head
    qkv = rng.normal(0, 1, (sum(lens), 3 * H))
    qkv[:, :H] *= 1.7
    qkv = qkv.astype(np.float16)
    qkv.setflags(write=False)
    return qkv


@functools.lru_cache(maxsize=None)
def op_reference(lens, n_head, d_head, kind, seed=0):
    """(W, want, bound) of op_inputs under draw_W(n_head, seed) for kernel `kind`, computed once per session"""
    W = draw_W(n_head, seed)
    qkv = op_inputs(lens, n_head, d_head)
    want, bnd = attention_packed(qkv.astype(np.float32) if kind == "f32" else qkv, lens, n_head, d_head, W, kind)
    return W, want, bnd


def cu_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# the whole model in float64
# ------------------------------------------------------------------------------------------------
class Model:
    """The dequantised tensors of a model file as float64 and the forward pass on them.  use_bias=False: the same encoder without the
    table (what the parent commit's library computes on a file without the tensor)."""

    def __init__(self, path, use_bias=True):
        self.mf = gf.read_model(path)
        self.hp = self.mf.hp
        self.t = {n: f8(self.mf.dequantized(n)) for n in self.mf.raw}
        self.W = self.t.get(gf.REL_BIAS_NAME) if use_bias else None

    def embed(self, ids):
        ids = np.asarray(ids)
        n = len(ids)
        pre = self.t["embeddings.word_embeddings.weight"][ids] + self.t["embeddings.token_type_embeddings.weight"][0] + \
            self.t["embeddings.position_embeddings.weight"][np.arange(n)]
        return layernorm(pre, self.t["embeddings.LayerNorm.weight"], self.t["embeddings.LayerNorm.bias"])

    def layer(self, x, i):
        t, p = self.t, f"encoder.layer.{i}."
        nh, dh = self.hp.n_head, self.hp.n_embd // self.hp.n_head
        q, k, v = (x @ t[p + f"attention.self.{w}.weight"].T + t[p + f"attention.self.{w}.bias"] for w in ("query", "key", "value"))
        ctx = np.empty_like(x)
        for h in range(nh):
            s = slice(h * dh, (h + 1) * dh)
            b = bias_matrix(self.W, h, len(x)) if self.W is not None else 0.0
            ctx[:, s] = attention(q[:, s], k[:, s], v[:, s], b)
        y = layernorm(x + ctx @ t[p + "attention.output.dense.weight"].T + t[p + "attention.output.dense.bias"],
                      t[p + "attention.output.LayerNorm.weight"], t[p + "attention.output.LayerNorm.bias"])
        ff = gelu(y @ t[p + "intermediate.dense.weight"].T + t[p + "intermediate.dense.bias"])
        return layernorm(y + ff @ t[p + "output.dense.weight"].T + t[p + "output.dense.bias"], t[p + "output.LayerNorm.weight"],
                         t[p + "output.LayerNorm.bias"])

    def hidden(self, ids):
        """[n_layer + 1][n][H]: the states behind the embedding LayerNorm and behind every layer"""
        xs = [self.embed(ids)]
        for i in range(self.hp.n_layer):
            xs.append(self.layer(xs[-1], i))
        return np.stack(xs)

    def pooled(self, ids):
        """mean over the tokens, L2-normalised: the context's default pooling"""
        y = self.hidden(ids)[-1].mean(axis=0)
        return y / np.linalg.norm(y)


def mpnet_state_dict(weights, pad_rows=2):
    """hf_mpnet_weights' inverse: this format's tensors under HuggingFace MPNet's names, the position table with pad_rows zero rows in
    front (HuggingFace's positions start at padding_idx + 1 = 2) and no token-type table."""
    inv = {ours: theirs for theirs, ours in gf._MPNET_LAYER_NAMES.items()}
    out = {}
    for name, a in weights.items():
        a = np.asarray(a, dtype=np.float32)
        if name == "embeddings.token_type_embeddings.weight":
            continue
        if name == "embeddings.position_embeddings.weight":
            a = np.concatenate([np.zeros((pad_rows, a.shape[1]), dtype=np.float32), a])
        if name.startswith("encoder.layer."):
            parts = name.split(".")
            mid = ".".join(parts[3:-1])
            name = ".".join(parts[:3] + [inv[mid], parts[-1]])
        out[name] = a
    return out


# the end-to-end models of test_gpu_rel_bias.py: name -> (hparams, ftype, lengths of the batch, cut to the position table)
E2E_SEED = 7
E2E_MODELS = {
    "h64-f32": (gf.BertHParams(512, 512, 64, 128, 2, 2), "f32", LENS),
    "h64-f16": (gf.BertHParams(512, 512, 64, 128, 2, 2), "f16", LENS),
    "h64-q4_0": (gf.BertHParams(512, 512, 64, 128, 2, 2), "q4_0", LENS),
    "h768-f16": (gf.BertHParams(512, 512, 768, 3072, 12, 2), "f16", LENS),
}


def e2e_sentences(name):
    hp, _, lens = E2E_MODELS[name]
    rng = np.random.default_rng(300 + len(name))
    return [rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in lens]


def row_error(got, want):
    """max |row - f64| / max |row| over the rows of [.., H] arrays"""
    got, want = f8(got), f8(want)
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())
