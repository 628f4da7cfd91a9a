"""The walk order of attention_mfma_kernel's persistent form (csrc/attention.hip) restated once, for the tests that assert their own launch
geometry (test_gpu_launch_geometry.py, test_gpu_rel_bias_edges.py, test_rel_bias_edges_host.py): which (sentence, head) items a workgroup
takes, and the grid rule of attention_mfma_grid for a device of `cus` compute units."""


def _item_of(v, items):
    """attention_mfma_kernel's item_of: the logical item (sentence n_head + head) that place v of the walk order takes"""
    q8, r8, xcd = items >> 3, items & 7, v & 7
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (v >> 3)


def _walks(grid, items):
    """per workgroup the items it walks, in order"""
    walks = [[_item_of(v, items) for v in range(g, items, grid)] for g in range(grid)]
    assert sorted(i for w in walks for i in w) == list(range(items))
    return walks


def persistent_grid(items, cus=256):
    """attention_mfma_grid's grid of the persistent form (max_len > 128) on a device of `cus` compute units (a multiple of 8)"""
    return min(cus, items // 8 * 8) if items >= 8 else items


def walk_lengths(lens, n_head, grid):
    """per workgroup the token counts of the items it walks, in order"""
    return [[lens[i // n_head] for i in w] for w in _walks(grid, len(lens) * n_head)]
