"""The LANE ORDER of a 32-token block of the hidden state, restated in NumPy: what model_kernel's full-window form passes between its
layers' tails and starts from (layer_tail.hip's XRES layout; misc_kernels.hip's embed_ln_lanes_kernel writes it).  Block k of a [T][H]
buffer holds tokens 32 k .. 32 k + 31 and is the 32 H halves from 32 k H on.  Fragment q < H / 16 is the KiB q of the block; lane
l = 32 hi + l31 owns 16 bytes at 16 l of it: features 16 q + 4 hi + {0..3}, then 16 q + 8 + 4 hi + {0..3}, of token 32 k + l31.
A helper module for test_lane_order_host.py and test_gpu_embed_lane_order.py, not a conftest."""
import numpy as np


def byte_offset(token: int, feature: int) -> int:
    """byte of (token 0..31 of its block, feature) inside the block"""
    q, j = divmod(feature, 16)
    upper, j = divmod(j, 8)                # the lane's second group of four: features 16 q + 8 ..
    hi, e = divmod(j, 4)
    return 1024 * q + 16 * (32 * hi + token) + 8 * upper + 2 * e


def block_index(H: int) -> np.ndarray:
    """[32, H] int: the half of the block that holds (token, feature)"""
    return np.array([[byte_offset(t, f) // 2 for f in range(H)] for t in range(32)], dtype=np.int64)


def to_rows(lanes: np.ndarray) -> np.ndarray:
    """a [T, H] buffer in lane order (T a multiple of 32) as row-major rows"""
    T, H = lanes.shape
    assert T % 32 == 0 and H % 16 == 0
    blocks = np.ascontiguousarray(lanes).reshape(T // 32, 32 * H)
    return blocks[:, block_index(H)].reshape(T, H)


def to_lanes(rows: np.ndarray) -> np.ndarray:
    T, H = rows.shape
    assert T % 32 == 0 and H % 16 == 0
    out = np.empty((T // 32, 32 * H), dtype=rows.dtype)
    out[:, block_index(H).reshape(-1)] = np.ascontiguousarray(rows).reshape(T // 32, 32 * H)
    return out.reshape(T, H)
