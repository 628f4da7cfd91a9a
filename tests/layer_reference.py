"""Float64 restatement of everything of an encoder layer behind the attention (reference bert.cpp:859-901), shared by the tests of
the one-launch layer tail (test_gpu_parity.py) and of the latency route's kernels (test_gpu_latency_kernels.py)."""
import numpy as np


def f8(a):
    return np.asarray(a).astype(np.float64)


def layernorm(v, g, b):
    mu = v.mean(axis=1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True)
    return (v - mu) / np.sqrt(var + 1e-5) * g + b


def gelu(u):
    return 0.5 * u * (1 + np.tanh(0.7978845608028654 * u * (1 + 0.044715 * u * u)))


def layer_tail(ctx, x, Wo, W1, W2, bo, g1, be1, b1, b2, g2, be2):
    """y = LayerNorm(ctx Wo^T + bo + x), out = LayerNorm(gelu(y W1^T + b1) W2^T + b2 + y), with the two roundings to f16 the device
    makes on the way: y (mat-mul input and residual) and the GELU'ed intermediate."""
    y = layernorm(f8(ctx) @ f8(Wo).T + bo + f8(x), g1, be1)
    y16 = f8(y.astype(np.float16))                       # the device keeps y in f16 (GEMM input and residual)
    gl = gelu(y16 @ f8(W1).T + b1)
    return layernorm(f8(gl.astype(np.float16)) @ f8(W2).T + b2 + y16, g2, be2)
