"""The partition file (bert_hip_index_partition_save / _load; the format is stated in include/bert_hip.h): a loaded partition is
the saved one — n_lists, centroid bits, lists, and every probed search's bits —, a load runs no assignment (a hand-written file's
lists are installed as they are), and a refused file leaves the index with the partition it had."""
import os
import struct

import numpy as np
import pytest

import probe_filter_data as pf
from index_reference import assert_same

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

DTYPES = pf.DTYPES


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def data():
    return pf.make_data()


@pytest.fixture(scope="module")
def cix(model, data):
    ix = model.index(dim=pf.DIM, dtype="f32")
    ix.add(data[1])
    yield ix
    ix.close()


def partition_file(centroids, list_ids, dim=None, n_lists=None, n_part=None, version=1, magic=b"BHIPPRT1"):
    c = np.ascontiguousarray(centroids, dtype="<f4")
    l = np.ascontiguousarray(list_ids, dtype="<i4")
    head = magic + struct.pack("<4I", version, c.shape[1] if dim is None else dim, len(c) if n_lists is None else n_lists,
                               len(l) if n_part is None else n_part) + b"\0" * 40
    assert len(head) == 64
    return head + c.tobytes() + l.tobytes()


def probed_all(ix, queries):
    return [ix.search_probed(queries, k, nprobe) for nprobe, k in ((1, 10), (3, 100), (12, 256))]


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip(model, data, dtype, tmp_path):
    queries = data[2]
    ix = pf.make_index(model, data, dtype)
    path, part = str(tmp_path / "x.idx"), str(tmp_path / "x.idx.part")
    ix.save(path)
    ix.save_partition(part)
    assert not os.path.exists(part + ".tmp")
    lists, cents, want = ix.partition_lists(), ix.centroids(), probed_all(ix, queries)
    raw = open(part, "rb").read()
    assert raw == partition_file(cents, lists[:pf.N])                 # the stated layout, byte for byte
    ix.close()
    ld = model.load_index(path)
    assert ld.n_lists == 0                                            # (the index file holds no partition)
    ld.load_partition(part)
    assert ld.n_lists == pf.NL and np.array_equal(ld.centroids().view(np.int32), cents.view(np.int32))
    got_lists = ld.partition_lists()
    assert np.array_equal(got_lists, lists) and (got_lists[pf.N:] == -1).all()      # the tail is still the tail
    for got, w in zip(probed_all(ld, queries), want):
        assert_same(got, w, (dtype, "loaded"))
    allow = np.arange(pf.SIZE) % 7 == 0
    probe = model_probe(model, data, 3)
    assert_same(ld.search_probed(queries, 10, 3, allow=allow), pf.probed_filtered_by_filter(ld, got_lists, probe, queries, 10, allow), (dtype, "loaded, filtered"))
    ld.close()


_PROBE = {}


def model_probe(model, data, nprobe):
    """[Q, nprobe]: the centroid index's search, once"""
    if nprobe not in _PROBE:
        c = model.index(dim=pf.DIM, dtype="f32")
        c.add(data[1])
        _PROBE[nprobe] = c.search(data[2], nprobe)[0]
        c.close()
    return _PROBE[nprobe]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_load_runs_no_assignment(model, cix, data, dtype, tmp_path):
    rows, dirs, queries, more, _ = data
    ix = model.index(dim=pf.DIM, dtype=dtype)
    ix.add(rows)
    ix.add(more[:100])
    # every one of the first 1400 rows in list 0, whatever an assignment would say; the 200 rows behind are the tail
    n_part = 1400
    part = str(tmp_path / "hand.part")
    with open(part, "wb") as f:
        f.write(partition_file(dirs, np.zeros(n_part, np.int32)))
    ix.load_partition(part)
    lists = ix.partition_lists()
    assert ix.n_lists == pf.NL and (lists[:n_part] == 0).all() and (lists[n_part:] == -1).all() and len(lists) == pf.N + 100
    probe = cix.search(queries, 1)[0]
    assert (probe[:, 0] == 0).any() and (probe[:, 0] != 0).any()     # (some queries scan everything assigned, some the tail alone)
    for k in (10, 256):
        assert_same(ix.search_probed(queries, k, 1), pf.probed_filtered_by_filter(ix, lists, probe, queries, k), (dtype, "hand-written", k))
    ix.close()


def test_refused_files_keep_the_partition(model, data, tmp_path, capfd):
    rows, dirs, queries, more, _ = data
    ix = pf.make_index(model, data, "i8")
    before_lists, before = ix.partition_lists(), ix.search_probed(queries, 10, 3)
    good_ids = np.zeros(pf.N, np.int32)
    nan = dirs.copy()
    nan[4, 9] = np.nan
    ids_hi, ids_neg = good_ids.copy(), good_ids.copy()
    ids_hi[77], ids_neg[1499] = pf.NL, -1
    good = partition_file(dirs, good_ids)
    cases = {
        "dim mismatch": partition_file(np.zeros((pf.NL, pf.DIM + 1), np.float32), good_ids),
        "n_part > size": partition_file(dirs, np.zeros(pf.SIZE + 1, np.int32)),
        "a list id equal to n_lists": partition_file(dirs, ids_hi),
        "a list id of -1": partition_file(dirs, ids_neg),
        "a NaN centroid": partition_file(nan, good_ids),
        "one byte short": good[:-1],
        "one byte long": good + b"\0",
        "wrong magic": partition_file(dirs, good_ids, magic=b"BHIPIDX1"),
    }
    for name, raw in cases.items():
        p = str(tmp_path / "bad.part")
        with open(p, "wb") as f:
            f.write(raw)
        capfd.readouterr()
        r = ix.lib.bert_hip_index_partition_load(ix.ix, os.fsencode(p))
        err = capfd.readouterr().err
        assert r in (-2, -3) and "bert_hip_index_partition_load" in err, (name, r, err)
        assert ix.n_lists == pf.NL and np.array_equal(ix.partition_lists(), before_lists), name
        assert_same(ix.search_probed(queries, 10, 3), before, name)
    capfd.readouterr()
    assert ix.lib.bert_hip_index_partition_load(ix.ix, os.fsencode(str(tmp_path / "none.part"))) == -3
    assert "bert_hip_index_partition_load" in capfd.readouterr().err and ix.n_lists == pf.NL
    with pytest.raises(RuntimeError, match="bert_hip_index_partition_load"):
        ix.load_partition(str(tmp_path / "none.part"))
    # and the good file is taken: the index now has its lists
    with open(str(tmp_path / "good.part"), "wb") as f:
        f.write(good)
    ix.load_partition(str(tmp_path / "good.part"))
    assert (ix.partition_lists()[:pf.N] == 0).all()
    ix.close()


def test_save_without_a_partition_is_refused(model, data, tmp_path, capfd):
    ix = model.index(dim=pf.DIM, dtype="f16")
    ix.add(data[0][:100])
    p = str(tmp_path / "no.part")
    capfd.readouterr()
    assert ix.lib.bert_hip_index_partition_save(ix.ix, os.fsencode(p)) == -2
    assert "bert_hip_index_partition_save" in capfd.readouterr().err
    assert not os.path.exists(p) and not os.path.exists(p + ".tmp")
    with pytest.raises(RuntimeError, match="-2"):
        ix.save_partition(p)
    # a refused load onto an index without a partition leaves it without one
    with open(p, "wb") as f:
        f.write(partition_file(data[1], np.zeros(101, np.int32)))
    assert ix.lib.bert_hip_index_partition_load(ix.ix, os.fsencode(p)) == -2 and ix.n_lists == 0
    ix.close()


@pytest.mark.parametrize("dtype", ["f16", "b1"])
def test_after_compact(model, data, dtype, tmp_path):
    queries = data[2]
    ix = pf.make_index(model, data, dtype)
    old = ix.compact()
    assert len(ix) == pf.SIZE - 40 and len(old) == len(ix)
    lists, want = ix.partition_lists(), probed_all(ix, queries)
    n_part = int((lists >= 0).sum())
    assert n_part == pf.N - 25 and (lists[:n_part] >= 0).all() and (lists[n_part:] == -1).all()
    part = str(tmp_path / "c.part")
    ix.save_partition(part)
    ix.partition(None)
    assert ix.n_lists == 0
    ix.load_partition(part)
    assert ix.n_lists == pf.NL and np.array_equal(ix.partition_lists(), lists)
    for got, w in zip(probed_all(ix, queries), want):
        assert_same(got, w, (dtype, "compacted"))
    ix.close()
