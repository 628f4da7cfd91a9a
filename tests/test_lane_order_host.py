"""tests/lane_order.py against the layout layer_tail.hip defines in words (XRES_IN / XRES_OUT): result fragment (n, s) of a 32-token
block -- lane (l31, hi): features 32 n + 16 s + 4 hi + {0..3, 8..11} of token l31 -- is 1 KiB, lane l = 32 hi + l31's 16 bytes at
((2 n + s) 64 + l) 16 of the block.  No GPU."""
import numpy as np
import pytest

import lane_order


@pytest.mark.parametrize("H", [256, 384])
def test_the_layout_is_a_bijection_onto_the_blocks_halves(H):
    idx = lane_order.block_index(H)
    assert idx.shape == (32, H)
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(32 * H))


# (token, feature) -> byte, worked out by hand from the comment's formula: fragment (n, s), lane (l31, hi), group g of four, element e
#   byte = ((2 n + s) 64 + 32 hi + l31) 16 + 8 g + 2 e     with feature = 32 n + 16 s + 8 g + 4 hi + e
HAND = [
    ((0, 0), 0),                  # n 0 s 0 hi 0 g 0 e 0
    ((0, 3), 6),                  # e 3
    ((0, 4), 512),                # hi 1: lane 32
    ((0, 8), 8),                  # g 1: the lane's second group
    ((0, 12), 520),               # hi 1 g 1
    ((5, 16), 1024 + 80),         # s 1: fragment 1, lane 5
    ((17, 100), 6 * 1024 + 49 * 16),              # 100 = 96 + 4: n 3 s 0 hi 1: fragment 6, lane 32 + 17
    ((9, 255), 15 * 1024 + 41 * 16 + 8 + 6),      # 255 = 224 + 16 + 8 + 4 + 3: fragment 15, lane 32 + 9, g 1 e 3
    ((31, 383), 24 * 1024 - 2),                   # the last half of a block at H = 384
]


@pytest.mark.parametrize("case", HAND)
def test_hand_written_offsets(case):
    (token, feature), byte = case
    assert lane_order.byte_offset(token, feature) == byte


def test_the_formula_as_written():
    for H in (256, 384):
        idx = lane_order.block_index(H)
        for n in range(H // 32):
            for s in range(2):
                for hi in range(2):
                    for l31 in (0, 1, 30, 31):
                        base = ((2 * n + s) * 64 + 32 * hi + l31) * 16
                        feats = [32 * n + 16 * s + 4 * hi + k for k in (0, 1, 2, 3, 8, 9, 10, 11)]
                        assert [2 * int(idx[l31, f]) for f in feats] == [base + 2 * k for k in range(8)]


@pytest.mark.parametrize("H", [256, 384])
def test_round_trip(H):
    rows = np.arange(96 * H).astype(np.uint16).reshape(96, H).view(np.float16)          # (every half another bit pattern)
    lanes = lane_order.to_lanes(rows)
    assert np.array_equal(lane_order.to_rows(lanes).view(np.uint16), rows.view(np.uint16))
    # block 1 starts at half 32 H, and its first 16 bytes are token 32's features 0..3, 8..11
    assert np.array_equal(lanes.view(np.uint16).reshape(-1)[32 * H:32 * H + 8], rows.view(np.uint16)[32, [0, 1, 2, 3, 8, 9, 10, 11]])
