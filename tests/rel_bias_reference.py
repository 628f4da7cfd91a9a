"""Test infrastructure of the relative position bias tests (test_rel_bias_host.py, test_gpu_rel_bias.py, test_rel_bias_edges_host.py,
test_gpu_rel_bias_edges.py — the only place for their references, bounds, inputs and model lists): MPNet's bucket function and the
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


def bias_matrix(W, h, n, wrong=None):
    """float64 b [n][n], b[i][j] = W[bucket(j - i)][h].  wrong: what a kernel with a mistake in the lookup would add instead, for the
    host tests that show the references can tell (test_rel_bias_edges_host.py): "negated" takes query - key, "off_by_one" j - i + 1."""
    i = np.arange(n)
    d = i[None, :] - i[:, None]
    d = {None: d, "negated": -d, "off_by_one": d + 1}[wrong]
    return f8(np.asarray(W)[bucket(d), h])


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
    to the scaled score rounds once, 2^-24 |score + b| (fused with the scaling: less); the rest with score + b in place of the score.
    (q, k, v [.., n][d], b [n][n]: leading axes are sentences of one length, bounded at once.)"""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape[-2:]
    scale = 1 / np.sqrt(d)
    kT = np.swapaxes(k, -1, -2)
    sc = q @ kT * scale + b
    mx = sc.max(axis=-1, keepdims=True)
    eps = (d + 3) * U32 * (np.abs(q) @ np.abs(kT)) * scale + U32 * np.abs(sc) + U32 * (mx - sc) + native_expf_rel(sc - mx)
    p = np.exp(sc - mx)
    L = p.sum(axis=-1, keepdims=True)
    w = p / L
    dw = w * eps + 2.0 ** -126 / L
    dw = dw + w * dw.sum(axis=-1, keepdims=True)
    want = w @ v
    return dw @ np.abs(v) + (3 * n + 2) * U32 * (w @ np.abs(v)) + ulp16(want), want


def f32_bound(q, k, v, b):
    """f32_reference.softmax_bound (f32_attention_kernel) with the bias, extended as naive_bound extends its own: + 2^-24 |score + b|.
    (Leading axes as in naive_bound.)"""
    q, k, v = f8(q), f8(k), f8(v)
    n, d = q.shape[-2:]
    scale = 1 / np.sqrt(d)
    kT = np.swapaxes(k, -1, -2)
    sc = q @ kT * scale + b
    mx = sc.max(axis=-1, keepdims=True)
    eps = (d + 3) * U32 * (np.abs(q) @ np.abs(kT)) * scale + U32 * np.abs(sc) + U32 * (mx - sc) + 2 * EXPF_ULP * U32
    p = np.exp(sc - mx)
    w = p / p.sum(axis=-1, keepdims=True)
    dw = w * eps + w * (w * eps).sum(axis=-1, keepdims=True)
    return dw @ np.abs(v) + (2 * n + 2) * U32 * (w @ np.abs(v)), w @ v


BOUNDS = {"mfma": mfma_bound, "naive": naive_bound, "f32": f32_bound}


def attention_packed(qkv, lens, n_head, d_head, W, kind, items=None, wrong=None):
    """qkv [T][3H] of packed sentences, W [32][n_head] (None: no bias) -> (float64 context rows [T][H], the bounds of kernel `kind`).
    items: only these (sentence n_head + head) items are computed, the rest stays 0 with a bound of 0; wrong: see bias_matrix."""
    H = n_head * d_head
    want, bnd = np.zeros((len(qkv), H)), np.zeros((len(qkv), H))
    items = None if items is None else set(int(i) for i in items)
    t0 = 0
    for s, n in enumerate(lens):
        for h in range(n_head):
            if items is not None and s * n_head + h not in items:
                continue
            sl = slice(h * d_head, (h + 1) * d_head)
            q, k, v = (qkv[t0:t0 + n, i * H:(i + 1) * H][:, sl] for i in range(3))
            b = bias_matrix(W, h, n, wrong) if W is not None else np.zeros((n, n))
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
# the structural edges (test_gpu_rel_bias_edges.py, test_rel_bias_edges_host.py)
# ------------------------------------------------------------------------------------------------
P_LONG = 1152                            # the longest sentence the matrix-core launcher takes at d_head 32, and the table for it
# beyond 512 tokens the 1024 prefetched table entries do not hold the window: the strided loop of the staging runs (600: 175 entries of
# it, 1025 and 1152: more than a round of the 512 threads)
LONG_LENS = (1152, 600, 1025)
# 13 sentences, 2 heads: 26 items on a grid of 24 (attention_walk.persistent_grid); workgroup 0 walks sentence 0 -> 1, workgroup 1
# sentence 2 -> 3.  d_head -> (P, lengths)
MOVING_WALK = {32: (P_LONG, (512, 5, 7, 1152, 129, 128, 300, 64, 257, 1, 1025, 600, 130)),
               64: (512, (512, 5, 7, 400, 129, 128, 300, 64, 257, 1, 511, 200, 130))}
# the result must not depend on P: (lengths, the P's tried) in the one-chunk form (n = P = 128 included) and in the persistent one
P_FREE = {"one chunk": ((1, 2, 64, 127, 128), (128, 129, 130, 513, 1152)), "persistent": ((129, 7, 300, 128, 2), (300, 301, 513, 1152))}
P_SMALL_LENS = (1, 2, 127, 128)          # bounded at P = 128
GENERIC_D_HEADS = (20, 96)               # no matrix-core kernel: the engine's generic attention, with the unscaled table
GENERIC_LENS = (1, 2, 9, 65, 130)
MANY = 65537                             # sentences of 2 tokens: the second slice of launch_attention_naive / launch_f32_attention

# hard values: name -> lengths.  lookup: Q = 0, the score is the bias alone.  rise / fall: W ~ N(0, 1) with W[15] (keys 91 and more
# behind the query) = -300 and W[31] (91 and more ahead) = +300, and the mirror image: for a query in the middle the chunk maximum moves
# by 300 natural units twice, through the bias alone.  loud: W ~ N(0, 40^2).
HARD_CASES = {"lookup": (9, 128, 300), "rise": (257, 512), "fall": (257, 512), "loud": (9, 128, 300)}


@functools.lru_cache(maxsize=None)
def hard_inputs(case, n_head, d_head):
    """(qkv [T][3H] f16, W [32][n_head] f32) of a hard-value case.  Read-only."""
    lens = HARD_CASES[case]
    qkv = op_inputs(lens, n_head, d_head)
    W = draw_W(n_head, seed=3, sigma={"lookup": W_SIGMA, "rise": 1.0, "fall": 1.0, "loud": 40.0}[case])
    if case == "lookup":
        qkv = qkv.copy()
        qkv[:, :n_head * d_head] = 0
    if case in ("rise", "fall"):
        W[15], W[31] = (-300.0, 300.0) if case == "rise" else (300.0, -300.0)
    qkv.setflags(write=False)
    W.setflags(write=False)
    return qkv, W


@functools.lru_cache(maxsize=None)
def reference(lens, n_head, d_head, kind, seed=0, case=None, wrong=None):
    """(qkv, W, want, bound) for kernel `kind`, computed once per session: op_inputs under draw_W(n_head, seed), or the hard-value
    case's own inputs (lens is then HARD_CASES[case]).  qkv is f16; the f32 kernel takes the same values as f32."""
    qkv, W = (op_inputs(lens, n_head, d_head), draw_W(n_head, seed)) if case is None else hard_inputs(case, n_head, d_head)
    want, bnd = attention_packed(qkv.astype(np.float32) if kind == "f32" else qkv, lens, n_head, d_head, W, kind, wrong=wrong)
    return qkv, W, want, bnd


@functools.lru_cache(maxsize=None)
def many_inputs(n_head=1, d_head=2):
    """qkv [2 MANY][3 H] f16 of MANY sentences of 2 tokens.  Q is narrow and the two values of a sentence lie at least 2 apart in every
    feature, so that no row's softmax is one-hot and no row hides a change of its weights: a wrong table entry shows in EVERY row."""
    rng = np.random.default_rng(MANY)
    H = n_head * d_head
    qkv = rng.normal(0, 1, (2 * MANY, 3 * H))
    qkv[:, :H] = np.clip(0.5 * qkv[:, :H], -0.5, 0.5)
    qkv[:, H:2 * H] = np.clip(qkv[:, H:2 * H], -2.0, 2.0)               # (|q . k| / sqrt(d) <= 1.5: two scores differ by at most 3 + the table's step)
    qkv[:, 2 * H:] = (1 + np.abs(qkv[:, 2 * H:])) * np.where(np.arange(2 * MANY) % 2, -1.0, 1.0)[:, None]
    qkv = qkv.astype(np.float16)
    qkv.setflags(write=False)
    return qkv


def many_reference(qkv, W, kind, wrong=None):
    """(want, bound) [2 MANY][d] of many_inputs (1 head) for kernel `kind` (naive or f32), all sentences at once"""
    d = qkv.shape[1] // 3
    q, k, v = (f8(qkv[:, i * d:(i + 1) * d]).reshape(-1, 2, d) for i in range(3))
    bnd, want = BOUNDS[kind](q, k, v, bias_matrix(W, 0, 2, wrong))
    return want.reshape(-1, d), bnd.reshape(-1, d)


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


# the end-to-end models of test_gpu_rel_bias_edges.py: name -> (hparams, ftype, the calls: the lengths of each eval_packed batch).
#   h64-p128-f16: the one-chunk form alone, P = 128;  h64-p1152-f16: the strided table loop through the engine;  h64-p1152-f32: the F32
#   route at 16 bytes of LDS per token;  h128-p640-f16: d_head 64, where the matrix cores refuse beyond 512 tokens and the engine falls
#   back to the generic kernel with the UNSCALED table (the first call; the second runs on the matrix cores);  h80-f16: d_head 20, the
#   generic attention always
E2E_EDGE_MODELS = {
    "h64-p128-f16": (gf.BertHParams(512, 128, 64, 128, 2, 2), "f16", ((1, 2, 64, 127, 128),)),
    "h64-p1152-f16": (gf.BertHParams(512, 1152, 64, 128, 2, 2), "f16", ((1152, 600, 129, 7),)),
    "h64-p1152-f32": (gf.BertHParams(512, 1152, 64, 128, 2, 2), "f32", ((1152, 600, 129, 7),)),
    "h128-p640-f16": (gf.BertHParams(512, 640, 128, 256, 2, 2), "f16", ((600, 130), (512, 130))),
    "h80-f16": (gf.BertHParams(512, 512, 80, 160, 4, 2), "f16", ((1, 9, 65, 130),)),
}


def edge_calls(name):
    """the calls of an edge model as lists of token arrays; a sentence of one length is the same sentence in every call"""
    hp, _, calls = E2E_EDGE_MODELS[name]
    rng = np.random.default_rng(500 + len(name))
    by_len = {n: rng.integers(0, hp.n_vocab, size=n).astype(np.int32) for n in sorted({n for c in calls for n in c})}
    return [[by_len[n] for n in c] for c in calls]


def row_error(got, want):
    """max |row - f64| / max |row| over the rows of [.., H] arrays"""
    got, want = f8(got), f8(want)
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())
