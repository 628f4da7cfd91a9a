"""The data and the yardstick of test_gpu_search_probe_filter.py, test_gpu_rescore_probed.py and test_gpu_partition_file.py.
Nothing here touches the GPU by itself.  The rows and the centroids are those of test_gpu_search_probe.py (the same generator and
draws): 1500 rows of dim 72, twelve centroids of which list 5 is longer than 512, list 7 is empty (its centroid is a copy of
centroid 3, and every tie goes to the smaller id) and the lengths are no multiples of 32.  The 33 queries are drawn as that
file draws them, but never around centroid 10 (or 7): in that file's own draw every non-empty list is some query's nearest, and
one of the allow-lists here is "the rows of a list that no query probes at nprobe = 1", which must not be empty.  1100 more rows
follow the partition: the tail starts at row 1500, no multiple of 32, and spans two 1024-row chunks."""
import numpy as np

from index_reference import assert_same, unit  # noqa: F401

DTYPES = ["f32", "f16", "i8", "b1"]
N, DIM, NL, LONG, EMPTY, UNPROBED = 1500, 72, 12, 5, 7, 10
N_MORE, Q = 1100, 33
SIZE = N + N_MORE


def make_data():
    """rows [N, DIM], centroids [NL, DIM], queries [Q, DIM], more [N_MORE, DIM], gone [40] (the rows to remove: 25 in the lists,
    15 in the tail)"""
    rng = np.random.default_rng(77)
    dirs = unit(rng.standard_normal((NL, DIM)))
    dirs[EMPTY] = dirs[3]
    of = np.concatenate([np.full(600, LONG), rng.choice([d for d in range(NL) if d not in (LONG, EMPTY)], 900)])
    rows = unit(dirs[of] + 0.06 * rng.standard_normal((N, DIM)))[rng.permutation(N)]
    rows[100:110] = rows[100]                                        # duplicates: equal scores, the id decides
    rng = np.random.default_rng(78)
    near = rng.choice([d for d in range(NL) if d not in (EMPTY, UNPROBED)], Q)
    queries = unit(dirs[near] + 0.1 * rng.standard_normal((Q, DIM)))
    more = unit(dirs[rng.integers(0, NL, N_MORE)] + 0.06 * rng.standard_normal((N_MORE, DIM)))
    more[50:55] = rows[100]                                          # the same duplicates in the tail
    gone = np.concatenate([rng.choice(N, 25, replace=False), N + rng.choice(N_MORE, 15, replace=False)]).astype(np.int32)
    lens = np.bincount(np.argmax(rows.astype(np.float64) @ dirs.astype(np.float64).T, axis=1), minlength=NL)
    assert lens[LONG] > 512 and lens[EMPTY] == 0 and lens[UNPROBED] > 0 and (lens % 32 != 0).any(), lens
    return rows, dirs, queries, more, gone


def make_index(model, data, dtype, partitioned=True):
    """the rows, partitioned (or not), then the tail, then the removals: SIZE rows, 40 of them removed"""
    rows, dirs, _, more, gone = data
    ix = model.index(dim=DIM, dtype=dtype)
    ix.add(rows)
    if partitioned:
        ix.partition(dirs)
    assert ix.add(more) == N
    assert ix.remove(gone) == len(gone)
    return ix


def allow_lists(lists, probe1):
    """name -> allow-list over SIZE rows (bool, or uint32 words where the words themselves are the case).  lists: the index's
    partition_lists(); probe1 [Q, 1]: the list each query probes at nprobe = 1"""
    ar = np.arange(SIZE)
    unprobed = [l for l in range(NL) if (lists == l).any() and l not in set(probe1.reshape(-1).tolist())]
    assert unprobed, ("every non-empty list is probed", np.unique(probe1))
    out = {
        "every 7th row": ar % 7 == 0,
        "a run across row 1500": (ar >= 1390) & (ar < 1655),
        "tail rows only": ar >= N,
        "an unprobed list only": lists == unprobed[0],
        "a single row": ar == 1234,
        "no row": np.zeros(SIZE, bool),
        "all ones, junk beyond size": np.full((SIZE + 31) // 32, 0xFFFFFFFF, np.uint32),
    }
    assert SIZE % 32 != 0                                            # (so the last word has bits beyond size)
    return out


def as_bool(allow):
    """the rows an allow-list of either kind permits"""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        return a
    return np.unpackbits(a.view(np.uint8), bitorder="little")[:SIZE].astype(bool)


def probed_filtered_by_filter(ix, lists, probe, queries, k, allow=None):
    """the contract through public calls: per query ONE filtered search whose allow-list is (the rows of the lists probe[q] names,
    plus the tail) AND the caller's list.  lists: ix.partition_lists(); probe [Q, nprobe]: the centroid index's search"""
    ids = np.empty((len(queries), k), np.int32)
    sc = np.empty((len(queries), k), np.float32)
    mine = np.ones(len(lists), bool) if allow is None else as_bool(allow)
    for i, q in enumerate(queries):
        own = ((lists == -1) | np.isin(lists, probe[i][probe[i] >= 0])) & mine
        ids[i], sc[i] = (a[0] for a in ix.search(q[None], k, allow=own))
    return ids, sc
