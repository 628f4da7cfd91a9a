"""The device entry points under stream capture and graph replay (include/bert_hip.h "stream capture and graphs").  Everything else in
the suite launches eagerly; here every *_device form is captured on one stream, instantiated and launched, and held to BIT EQUALITY with
the eager call on the same buffers — the eager path is what the other files hold to float64 references.  Output buffers are refilled
with NaN (ids: -1) before every launch, eager or replayed.  A graph is launched at most 4 times; no capture forks onto a second
stream.  The helper is hip_graph.py."""
import subprocess
import sys

import numpy as np
import pytest

import hip_graph
import test_gpu_pooling as P
from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from conftest import ROOT, cosine
from test_gpu_parity import MIN_COS

pytestmark = pytest.mark.gpu

OK = hip_graph.HIP_SUCCESS


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


@pytest.fixture(scope="module")
def tiny(make_model):
    path, hp = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m, hp
    m.close()


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _replay(hip, graph_exec, stream, outputs):
    """outputs: [(pointer, shape, dtype)], poisoned, then one launch; returns their contents"""
    for p, shape, dtype in outputs:
        hip.poison(p, shape, dtype)
    hip.launch(graph_exec, stream)
    return [hip.download(p, shape, dtype) for p, shape, dtype in outputs]


def _eager(hip, call, outputs):
    for p, shape, dtype in outputs:
        hip.poison(p, shape, dtype)
    assert call() == 0
    return [hip.download(p, shape, dtype) for p, shape, dtype in outputs]


def _captured(hip, stream, call, outputs, want_nodes=None):
    """call() under capture on stream: it returns 0, the capture ends with hipSuccess, nothing ran (the poisoned outputs are as they
    were).  Returns (graph, exec)."""
    for p, shape, dtype in outputs:
        hip.poison(p, shape, dtype)
    with hip.capture(stream) as cap:
        r = call()
    assert r == 0 and cap.status == OK and cap.graph, (r, cap.status, cap.graph)
    for p, shape, dtype in outputs:
        got = hip.download(p, shape, dtype)
        assert (got == -1).all() if np.issubdtype(dtype, np.integer) else np.isnan(got).all(), "capturing must run nothing"
    nodes = hip.kernel_nodes(cap.graph)
    assert nodes > 0 and (want_nodes is None or nodes == want_nodes), (nodes, want_nodes)
    return cap.graph, hip.instantiate(cap.graph)


def _all_same(got, want, what):
    for g, w in zip(got, want):
        assert _same(g, w), what


# ------------------------------------------------------------------------------------------------
# the forward pass, once per route
# ------------------------------------------------------------------------------------------------
def _batches(name, hp):
    """(first batch, second batch, over-long cu): the second has other ids and the lengths in reverse order — the same sum and maximum,
    no sentence boundary in common —; the third cu has the same T with the last sentence one token longer than max_len."""
    sents = P._sentences(name, hp)
    lens = [len(s) for s in sents]
    second = [gf.synthetic_token_ids(1, n, hp.n_vocab, seed=9000 + i)[0] for i, n in enumerate(reversed(lens))]
    cu1, cu2 = _cu(lens), _cu(lens[::-1])
    assert not set(cu1[1:-1]) & set(cu2[1:-1]) and cu1[-1] == cu2[-1]
    long_lens = lens[:-2] + [lens[-2] - 1, lens[-1] + 1]
    assert lens[-1] == max(lens) and lens[-2] > 1
    return (np.concatenate(sents).astype(np.int32), cu1), (np.concatenate(second).astype(np.int32), cu2), _cu(long_lens)


@pytest.mark.parametrize("arm", list(P.ARMS))
def test_forward_pass_replays_with_the_eager_bits(arm, make_model, model_dir, hip):
    name, options, _, _ = P.ARMS[arm]
    path, hp = P._model_file(name, make_model, model_dir)
    (toks, cu), (toks2, cu2), cu_long = _batches(name, hp)
    B, T, H, max_len = len(cu) - 1, int(cu[-1]), hp.n_embd, int(np.diff(cu).max())
    lib = pybert.lib()
    m = pybert.BertModel(path)
    for k, v in options.items():
        m.set_option(k, v)
    host = m.eval_packed(toks, cu)
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.nans((B, H))
    out = [(d_out, (B, H), np.float32)]
    s, s2 = hip.stream(), hip.stream()
    m.reserve(T, B)

    def call(stream):
        return lambda: lib.bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max_len, d_out, stream)

    (E,) = _eager(hip, call(s), out)
    assert m.check() == 0 and _same(E, host)
    # the launches of the eager call, by the engine's own count: a launch that went to another stream would be missing from the graph
    m.profile(True)
    (timed,) = _eager(hip, call(s), out)
    n_launches = sum(v["launches"] for v in m.profile_report().values())
    m.profile(False)
    assert _same(timed, E) and n_launches > 0
    graph, ex = _captured(hip, s, call(s), out, want_nodes=n_launches)
    for i in range(3):
        (got,) = _replay(hip, ex, s, out)
        assert _same(got, E), (arm, "replay", i)
    assert m.check() == 0
    if arm in ("one_launch", "f32"):
        # (not bit equality alone: the replayed rows against the oracle, by test_gpu_pooling's rule for the default mode)
        want = P.reference(name, make_model, model_dir)[3][P.MODES[0]]
        for b in range(B):
            c = cosine(got[b], want[b])
            assert c > MIN_COS[P.MODELS[name][1]] and abs(np.linalg.norm(got[b].astype(np.float64)) - 1) < 1e-5, (arm, b, c)
    # another batch of the same (B, T, max_len) in the same buffers: the lengths exist only in HBM, nothing of them is in the graph
    hip.write(d_t, toks2)
    hip.write(d_cu, cu2)
    (got2,) = _replay(hip, ex, s, out)
    (E2,) = _eager(hip, call(s), out)
    assert m.check() == 0 and _same(got2, E2) and not _same(E2, E), arm
    # a sentence longer than max_len: its row NaN, the others finite, the status word set once
    hip.write(d_cu, cu_long)
    (bad,) = _replay(hip, ex, s, out)
    assert np.isnan(bad[B - 1]).all() and np.isfinite(bad[:B - 1]).all(), arm
    assert m.check() == 1 and m.check() == 0
    hip.destroy(ex, graph)
    # after the capture, every eager entry point as before
    hip.write(d_t, toks)
    hip.write(d_cu, cu)
    for stream in (s2, 0):
        (again,) = _eager(hip, call(stream), out)
        assert _same(again, E), (arm, "eager after the capture, stream", stream)
    assert _same(m.eval_packed(toks, cu), E) and m.check() == 0
    hip.sync()
    hip.destroy_stream(s)
    hip.destroy_stream(s2)
    hip.free(d_t, d_cu, d_out)
    m.close()


# ------------------------------------------------------------------------------------------------
# token rows, MaxSim and grouped pooling
# ------------------------------------------------------------------------------------------------
def _ids(hp, lens, seed):
    return np.concatenate([gf.synthetic_token_ids(1, n, hp.n_vocab, seed=seed + i)[0] for i, n in enumerate(lens)]).astype(np.int32)


def test_token_rows_twice_and_maxsim_in_one_graph(tiny, hip):
    """Three operations of one context in one capture: the second and the third follow the first on the stream alone."""
    m, hp = tiny
    lib, H = m.lib, hp.n_embd
    qlens, dlens = [1, 31, 33], [32, 33, 64, 7]
    qcu, dcu = _cu(qlens), _cu(dlens)
    Tq, Td = int(qcu[-1]), int(dcu[-1])
    d_qt, d_qcu, d_dt, d_dcu = hip.upload(_ids(hp, qlens, 10)), hip.upload(qcu), hip.upload(_ids(hp, dlens, 20)), hip.upload(dcu)
    d_qrows, d_drows, d_qemb, d_sc = hip.nans((Tq, H), np.float16), hip.nans((Td, H), np.float16), hip.nans((3, H)), hip.nans((3, 4))
    out = [(d_qrows, (Tq, H), np.float16), (d_drows, (Td, H), np.float16), (d_qemb, (3, H), np.float32), (d_sc, (3, 4), np.float32)]
    s = hip.stream()
    m.reserve(Td, 4)

    def chain():
        r = lib.bert_hip_eval_packed_tokens_device(m.ctx, d_qt, d_qcu, 3, Tq, max(qlens), 3, d_qrows, d_qemb, s)
        r = r or lib.bert_hip_eval_packed_tokens_device(m.ctx, d_dt, d_dcu, 4, Td, max(dlens), 3, d_drows, None, s)
        return r or lib.bert_hip_maxsim_device(m.ctx, d_qrows, d_qcu, 3, d_drows, d_dcu, 4, H, None, 0, 0, d_sc, s)

    E = _eager(hip, chain, out)
    assert m.check() == 0 and all(np.isfinite(e.astype(np.float32)).all() for e in E)
    graph, ex = _captured(hip, s, chain, out)
    _all_same(_replay(hip, ex, s, out), E, "replay")
    hip.write(d_qt, _ids(hp, qlens, 30))
    hip.write(d_dt, _ids(hp, dlens, 40))
    got = _replay(hip, ex, s, out)
    E2 = _eager(hip, chain, out)
    _all_same(got, E2, "replay after new ids")
    assert not _same(E2[3], E[3]) and m.check() == 0
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_qt, d_qcu, d_dt, d_dcu, d_qrows, d_drows, d_qemb, d_sc)


def test_grouped_pooling_replays(tiny, hip):
    m, hp = tiny
    lib, H = m.lib, hp.n_embd
    lens, gcu = [32, 33, 64, 7], np.array([0, 1, 3, 4], np.int32)
    cu = _cu(lens)
    T, B, G = int(cu[-1]), len(lens), len(gcu) - 1
    d_t, d_cu, d_g, d_out = hip.upload(_ids(hp, lens, 50)), hip.upload(cu), hip.upload(gcu), hip.nans((G, H))
    out = [(d_out, (G, H), np.float32)]
    s = hip.stream()
    m.reserve(T, B)
    call = lambda: lib.bert_hip_eval_packed_grouped_device(m.ctx, d_t, d_cu, B, T, max(lens), d_g, G, d_out, s)
    E = _eager(hip, call, out)                      # (the raw rows' buffer is not reserve's: the first call at the shape sizes it)
    assert m.check() == 0 and np.isfinite(E[0]).all()
    graph, ex = _captured(hip, s, call, out)
    _all_same(_replay(hip, ex, s, out), E, "replay")
    hip.write(d_t, _ids(hp, lens, 60))
    got = _replay(hip, ex, s, out)
    E2 = _eager(hip, call, out)
    _all_same(got, E2, "replay after new ids")
    assert not _same(E2[0], E[0]) and m.check() == 0
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_g, d_out)


def _maxsim_1024(rng):
    """synthetic f16 rows at H = 1024 (the launch with more than 64 KiB of LDS), the list form"""
    qcu, dcu = _cu([3, 40]), _cu([5, 70, 33])
    q = (rng.standard_normal((int(qcu[-1]), 1024)) / 32).astype(np.float16)
    d = (rng.standard_normal((int(dcu[-1]), 1024)) / 32).astype(np.float16)
    pairs = np.array([[0, 0], [1, 2], [1, 1], [0, 2], [1, 1]], np.int32)
    return q, qcu, d, dcu, pairs


def test_maxsim_at_h_1024_replays(tiny, hip):
    m, _ = tiny
    q, qcu, d, dcu, pairs = _maxsim_1024(np.random.default_rng(1024))
    d_q, d_qcu, d_d, d_dcu, d_p, d_sc = hip.upload(q), hip.upload(qcu), hip.upload(d), hip.upload(dcu), hip.upload(pairs), hip.nans(len(pairs))
    out = [(d_sc, (len(pairs),), np.float32)]
    s = hip.stream()
    call = lambda: m.lib.bert_hip_maxsim_device(m.ctx, d_q, d_qcu, 2, d_d, d_dcu, 3, 1024, d_p, len(pairs), 1, d_sc, s)
    E = _eager(hip, call, out)
    assert np.isfinite(E[0]).all() and E[0][2] == E[0][4]
    graph, ex = _captured(hip, s, call, out, want_nodes=1)
    _all_same(_replay(hip, ex, s, out), E, "replay")
    hip.write(d_q, q[::-1])
    got = _replay(hip, ex, s, out)
    E2 = _eager(hip, call, out)
    _all_same(got, E2, "replay after new rows")
    assert not _same(E2[0], E[0])
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qcu, d_d, d_dcu, d_p, d_sc)


# ------------------------------------------------------------------------------------------------
# the index
# ------------------------------------------------------------------------------------------------
DIM, N, Q, K = 130, 4500, 33, 10          # padding in every row form, more than one slice
DTYPES = ["f32", "f16", "i8", "b1"]


def _index_data():
    rng = np.random.default_rng(130)
    return _unit_rows(rng, N, DIM), _unit_rows(rng, 3000, DIM), _unit_rows(rng, Q, DIM), _unit_rows(rng, Q, DIM)


def _make(m, dtype, rows, reserve=(6000, Q, K)):
    ix = m.index(dim=DIM, dtype=dtype)
    ix.reserve(*reserve)
    assert ix.add(rows) == 0
    return ix


@pytest.mark.parametrize("dtype", DTYPES)
def test_index_search_replays_and_the_index_works_afterwards(tiny, hip, dtype, tmp_path):
    m, _ = tiny
    lib = m.lib
    rows, more, q1, q2 = _index_data()
    ix, twin = _make(m, dtype, rows), _make(m, dtype, rows)          # (the twin is never captured)
    d_q, d_ids, d_sc = hip.upload(q1), hip.nans((Q, K), np.int32), hip.nans((Q, K))
    out = [(d_ids, (Q, K), np.int32), (d_sc, (Q, K), np.float32)]
    s = hip.stream()
    search = lambda: lib.bert_hip_index_search_device(ix.ix, Q, d_q, K, d_ids, d_sc, s)
    E = _eager(hip, search, out)
    _all_same(E, twin.search(q1, K), "device against host")
    graph, ex = _captured(hip, s, search, out)
    _all_same(_replay(hip, ex, s, out), E, "replay")
    hip.write(d_q, q2)
    got = _replay(hip, ex, s, out)
    E2 = _eager(hip, search, out)
    _all_same(got, E2, "replay after new queries")
    assert not np.array_equal(E2[0], E[0])
    # the allow-list lives in HBM: its bits may change between replays
    n_words = (N + 31) // 32
    allow = np.arange(N) % 3 == 0
    d_allow = hip.upload(pybert.allow_words(allow, N))
    filtered = lambda: lib.bert_hip_index_search_filtered_device(ix.ix, Q, d_q, K, d_allow, n_words, d_ids, d_sc, s)
    F = _eager(hip, filtered, out)
    assert (F[0] % 3 == 0).all()
    fgraph, fex = _captured(hip, s, filtered, out)
    _all_same(_replay(hip, fex, s, out), F, "filtered replay")
    for step, allow in enumerate((np.arange(N) % 3 == 1, np.arange(N) >= N - 7)):
        hip.write(d_allow, pybert.allow_words(allow, N))
        got = _replay(hip, fex, s, out)
        F2 = _eager(hip, filtered, out)
        _all_same(got, F2, ("filtered replay, new bits", step))
        assert allow[F2[0][F2[0] >= 0]].all() and (step == 0 or (F2[0][:, 7:] == -1).all())
    hip.destroy(ex, graph)          # (one graph destroyed, the other still alive: neither may matter to what follows)
    # everything that blocks on the index's event, against the index that was never captured
    for x in (ix, twin):
        assert x.add(more) == N and len(x) == N + 3000          # beyond the reserved 6000: the storage grows
    _all_same(ix.search(q1, K), twin.search(q1, K), "search after growing")
    gone = np.arange(5, N + 3000, 11, dtype=np.int32)
    for x in (ix, twin):
        assert x.remove(gone) == len(gone)
    got = ix.search(q2, K)
    _all_same(got, twin.search(q2, K), "search after remove")
    assert not np.isin(got[0], gone).any()
    old = [x.compact() for x in (ix, twin)]
    assert np.array_equal(old[0], old[1]) and len(ix) == N + 3000 - len(gone)
    _all_same(ix.search(q1, K), twin.search(q1, K), "search after compact")
    path = str(tmp_path / f"captured_{dtype}.idx")
    ix.save(path)
    loaded = m.load_index(path)
    _all_same(loaded.search(q2, K), twin.search(q2, K), "search of the loaded index")
    hip.destroy(fex, fgraph)
    hip.destroy_stream(s)
    hip.free(d_q, d_ids, d_sc, d_allow)
    for x in (ix, twin, loaded):
        x.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_device_and_search_in_one_capture(tiny, hip, dtype):
    """What the header says of add_device under capture: the first id is returned and the size grows when the call is CAPTURED; the rows
    arrive with each launch, at the place fixed then."""
    m, _ = tiny
    lib = m.lib
    rows, more, q1, _ = _index_data()
    new = more[:64]
    ix = _make(m, dtype, rows)
    want = _make(m, dtype, np.concatenate([rows, new])).search(q1, K)
    d_new, d_q, d_ids, d_sc = hip.upload(new), hip.upload(q1), hip.nans((Q, K), np.int32), hip.nans((Q, K))
    out = [(d_ids, (Q, K), np.int32), (d_sc, (Q, K), np.float32)]
    s = hip.stream()
    first = []

    def add_then_search():
        first.append(lib.bert_hip_index_add_device(ix.ix, 64, d_new, s))
        return lib.bert_hip_index_search_device(ix.ix, Q, d_q, K, d_ids, d_sc, s)

    graph, ex = _captured(hip, s, add_then_search, out)
    assert first == [N] and len(ix) == N + 64
    got = _replay(hip, ex, s, out)
    _all_same(got, want, "add + search, first launch")
    _all_same(_replay(hip, ex, s, out), got, "add + search, second launch")
    _all_same(ix.search(q1, K), want, "host search afterwards")
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_new, d_q, d_ids, d_sc)
    ix.close()


@pytest.mark.parametrize("coarse_dtype,fine_dtype", [("b1", "f16"), ("i8", "f32")])
def test_rescore_probed_and_two_stage_forms_replay(tiny, hip, coarse_dtype, fine_dtype):
    m, _ = tiny
    lib = m.lib
    rows, more, q1, q2 = _index_data()
    n_lists, nprobe, n_cand = 8, 3, 50
    coarse, fine = _make(m, coarse_dtype, rows, (N, Q, n_cand)), _make(m, fine_dtype, rows, (N, Q, K))
    coarse.partition(rows[np.random.default_rng(8).choice(N, n_lists, replace=False)])
    assert coarse.n_lists == n_lists
    cand = coarse.search(q1, n_cand)[0]
    n_words = (N + 31) // 32
    d_q, d_cand, d_allow = hip.upload(q1), hip.upload(cand), hip.upload(pybert.allow_words(np.arange(N) % 2 == 0, N))
    d_ids, d_sc = hip.nans((Q, K), np.int32), hip.nans((Q, K))
    out = [(d_ids, (Q, K), np.int32), (d_sc, (Q, K), np.float32)]
    s = hip.stream()
    forms = {
        "rescore_device": lambda: lib.bert_hip_index_rescore_device(fine.ix, Q, d_q, n_cand, d_cand, K, d_ids, d_sc, s),
        "search_probed_device": lambda: lib.bert_hip_index_search_probed_device(coarse.ix, Q, d_q, nprobe, K, d_ids, d_sc, s),
        "search_probed_filtered_device": lambda: lib.bert_hip_index_search_probed_filtered_device(coarse.ix, Q, d_q, nprobe, K, d_allow, n_words, d_ids, d_sc, s),
        "search_rescored_device": lambda: lib.bert_hip_index_search_rescored_device(coarse.ix, fine.ix, Q, d_q, n_cand, K, d_ids, d_sc, s),
        "search_rescored_probed_device": lambda: lib.bert_hip_index_search_rescored_probed_device(coarse.ix, fine.ix, Q, d_q, nprobe, n_cand, K, d_allow, n_words,
                                                                                               d_ids, d_sc, s),
    }
    host = {
        "rescore_device": lambda q: fine.rescore(q, cand, K),
        "search_probed_device": lambda q: coarse.search_probed(q, K, nprobe),
        "search_probed_filtered_device": lambda q: coarse.search_probed(q, K, nprobe, allow=np.arange(N) % 2 == 0),
        "search_rescored_device": lambda q: coarse.search_rescored(fine, q, K, n_cand),
        "search_rescored_probed_device": lambda q: coarse.search_rescored_probed(fine, q, K, n_cand, nprobe, allow=np.arange(N) % 2 == 0),
    }
    graphs = []
    for name, call in forms.items():
        hip.write(d_q, q1)
        E = _eager(hip, call, out)                  # (the header's advice: once at the shape before a capture)
        _all_same(E, host[name](q1), (name, "device against host"))
        assert (E[0] >= 0).any()
        graph, ex = _captured(hip, s, call, out)
        graphs.append((ex, graph))
        _all_same(_replay(hip, ex, s, out), E, (name, "replay"))
        hip.write(d_q, q2)
        _all_same(_replay(hip, ex, s, out), host[name](q2), (name, "replay after new queries"))
    for ex, graph in graphs:
        hip.destroy(ex, graph)
    # both indexes still grow beyond their capacity, and find the new rows
    for x in (coarse, fine):
        assert x.add(more[:100]) == N and len(x) == N + 100
    assert np.array_equal(fine.search(more[:5], 1)[0].ravel(), N + np.arange(5))
    assert coarse.search_probed(more[:5], K, nprobe)[0].shape == (5, K)
    hip.destroy_stream(s)
    hip.free(d_q, d_cand, d_allow, d_ids, d_sc)
    coarse.close()
    fine.close()


def test_encode_and_search_in_one_graph(make_model, hip):
    """test_gpu_search.py's forward pass -> search on one stream, captured: eval_packed_device into d_emb, search_device(d_emb)."""
    path, hp = make_model("minilm-l6", "f16", 0)
    m = pybert.BertModel(path)
    lib, H = m.lib, hp.n_embd
    rng = np.random.default_rng(5)
    dlens = rng.integers(5, 60, 200)
    docs = m.eval_packed(rng.integers(1000, hp.n_vocab, size=int(dlens.sum())).astype(np.int32), _cu(dlens))
    ix = m.index(dtype="f16")
    ix.reserve(len(docs), 5, K)
    ix.add(docs)
    lens = [7, 33, 12, 64, 20]
    cu = _cu(lens)
    B, T = len(lens), int(cu[-1])
    d_t, d_cu, d_emb = hip.upload(_ids(hp, lens, 70)), hip.upload(cu), hip.nans((B, H))
    d_ids, d_sc = hip.nans((B, K), np.int32), hip.nans((B, K))
    out = [(d_emb, (B, H), np.float32), (d_ids, (B, K), np.int32), (d_sc, (B, K), np.float32)]
    s = hip.stream()
    m.reserve(T, B)

    def pair():
        return lib.bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max(lens), d_emb, s) or lib.bert_hip_index_search_device(ix.ix, B, d_emb, K, d_ids, d_sc, s)

    E = _eager(hip, pair, out)
    assert m.check() == 0
    _all_same(E[1:], ix.search(E[0], K), "device against host")
    graph, ex = _captured(hip, s, pair, out)
    _all_same(_replay(hip, ex, s, out), E, "replay")
    hip.write(d_t, _ids(hp, lens, 80))
    got = _replay(hip, ex, s, out)
    E2 = _eager(hip, pair, out)
    _all_same(got, E2, "replay after new ids")
    assert not _same(E2[0], E[0]) and m.check() == 0
    hip.destroy(ex, graph)
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_emb, d_ids, d_sc)
    m.close()


# ------------------------------------------------------------------------------------------------
# the first pass of a process, captured
# ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import hip_graph
from bert_cpp_amd import pybert
import test_gpu_stream_capture as T
z = np.load(sys.argv[2])
hip = hip_graph.Hip()
s = hip.stream()
runs = []
for arm, path in zip(("one_launch", "latency", "folded"), sys.argv[3:6]):
    toks, cu = z[arm + "_toks"], z[arm + "_cu"]
    m = pybert.BertModel(path)
    for k, v in T.P.ARMS[arm][1].items():
        m.set_option(k, v)
    B, n, max_len = len(cu) - 1, int(cu[-1]), int(np.diff(cu).max())
    m.reserve(n, B)
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.nans((B, m.n_embd))
    call = lambda m=m, a=(d_t, d_cu, B, n, max_len, d_out): m.lib.bert_hip_eval_packed_device(m.ctx, *a, s)
    runs.append((arm, m, call, [(d_out, (B, m.n_embd), np.float32)]))
q, qcu, d, dcu, pairs = T._maxsim_1024(np.random.default_rng(1024))
d_sc = hip.nans(len(pairs))
args = (hip.upload(q), hip.upload(qcu), 2, hip.upload(d), hip.upload(dcu), 3, 1024, hip.upload(pairs), len(pairs), 1, d_sc, s)
m0 = runs[0][1]
runs.append(("maxsim", m0, lambda: m0.lib.bert_hip_maxsim_device(m0.ctx, *args), [(d_sc, (len(pairs),), np.float32)]))
# the first launches of the process are captured ones: no kernel has run, no one-time opt-in has been made
graphs = [T._captured(hip, s, call, out) for _, _, call, out in runs]
replayed = [T._replay(hip, ex, s, out) for (_, ex), (_, _, _, out) in zip(graphs, runs)]
for (arm, m, call, out), got in zip(runs, replayed):
    want = T._eager(hip, call, out)
    assert all(np.isfinite(w).all() for w in want), arm
    T._all_same(got, want, arm)
    assert m.check() == 0, arm
print("first pass under capture ok")
"""


def test_first_pass_of_a_process_under_capture(make_model, model_dir, tmp_path):
    """The one-time opt-ins (hipFuncSetAttribute behind configure_once) and the lazy device queries are process-wide: a fresh child whose
    first device calls, and the H = 1024 MaxSim, are captured; the eager results are computed afterwards."""
    arms = ("one_launch", "latency", "folded")
    paths, batch = [], {}
    for arm in arms:
        name = P.ARMS[arm][0]
        path, hp = P._model_file(name, make_model, model_dir)
        sents = P._sentences(name, hp)
        paths.append(path)
        batch[arm + "_toks"], batch[arm + "_cu"] = np.concatenate(sents).astype(np.int32), _cu([len(s) for s in sents])
    npz = str(tmp_path / "batches.npz")
    np.savez(npz, **batch)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, npz] + paths, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0 and "first pass under capture ok" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------
# profiling excludes capture; an allocation under capture
# ------------------------------------------------------------------------------------------------
def test_profiling_refuses_a_capturing_stream(tiny, hip, capfd):
    m, hp = tiny
    lib, H = m.lib, hp.n_embd
    lens = [5, 64, 33]
    cu = _cu(lens)
    B, T = len(lens), int(cu[-1])
    rows, _, q1, _ = _index_data()
    ix = _make(m, "f16", rows)
    d_t, d_cu, d_out = hip.upload(_ids(hp, lens, 90)), hip.upload(cu), hip.nans((B, H))
    d_q, d_ids, d_sc = hip.upload(q1), hip.nans((Q, K), np.int32), hip.nans((Q, K))
    mq, mqcu, md, mdcu, mp = _maxsim_1024(np.random.default_rng(7))
    d_ms = hip.nans(len(mp))
    mptr = [hip.upload(a) for a in (mq, mqcu, md, mdcu, mp)]
    margs = (mptr[0], mptr[1], 2, mptr[2], mptr[3], 3, 1024, mptr[4], len(mp), 1, d_ms)
    s = hip.stream()
    m.reserve(T, B)
    calls = {
        "bert_hip_eval_packed_device": (lambda: lib.bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max(lens), d_out, s), [(d_out, (B, H), np.float32)]),
        "bert_hip_index_search_device": (lambda: lib.bert_hip_index_search_device(ix.ix, Q, d_q, K, d_ids, d_sc, s),
                                         [(d_ids, (Q, K), np.int32), (d_sc, (Q, K), np.float32)]),
        "bert_hip_maxsim_device": (lambda: lib.bert_hip_maxsim_device(m.ctx, *margs, s), [(d_ms, (len(mp),), np.float32)]),
    }
    eager = {name: _eager(hip, call, out) for name, (call, out) in calls.items()}
    m.profile(True)
    m.profile_report()
    for name, (call, out) in calls.items():
        capfd.readouterr()
        with hip.capture(s) as cap:
            r = call()
        err = capfd.readouterr().err
        assert r < 0, (name, r)
        assert len(err.splitlines()) == 1 and name in err and "profil" in err, (name, err)
        assert cap.status == OK and (not cap.graph or hip.kernel_nodes(cap.graph) == 0), (name, cap.status)
        if cap.graph:
            hip.destroy(graph=cap.graph)
    assert m.profile_report(families=True) == {}
    # eager calls are still timed, and with profiling off the capture works
    _all_same(_eager(hip, calls["bert_hip_eval_packed_device"][0], calls["bert_hip_eval_packed_device"][1]), eager["bert_hip_eval_packed_device"], "timed eager")
    assert "pool_normalize" in m.profile_report()
    m.profile(False)
    for name, (call, out) in calls.items():
        graph, ex = _captured(hip, s, call, out)
        _all_same(_replay(hip, ex, s, out), eager[name], (name, "replay with profiling off"))
        hip.destroy(ex, graph)
    assert m.check() == 0
    hip.destroy_stream(s)
    hip.free(d_t, d_cu, d_out, d_q, d_ids, d_sc, d_ms, *mptr)
    ix.close()


def test_an_allocation_under_capture_is_noticed(make_model, hip, capfd):
    """The control: a fresh context WITHOUT bert_hip_reserve, so the device form has to size its workspace inside the capture, which
    the header calls illegal.  Run once, not repeated.  Seen on the MI355X (HIP 7.2): the call returns -3 after "hipMalloc(&p, n):
    operation not permitted when stream is capturing" (hipErrorStreamCaptureUnsupported, 900); hipStreamEndCapture returns
    hipErrorStreamCaptureInvalidated (901) and no graph.  The context is unharmed: the host entry points, eager device calls on other
    streams and on the null stream, and a clean capture on another stream all work.  The stream of the broken capture is not: the
    runtime goes on reporting it as invalidated (hipStreamIsCapturing: 2; a second hipStreamEndCapture: 908), and an eager call on it
    fails with 901 — it can only be destroyed.  The header says so; the last point is the runtime's and is not asserted here."""
    path, hp = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    lens = [5, 64, 33]
    cu = _cu(lens)
    B, T, H = len(lens), int(cu[-1]), hp.n_embd
    toks = _ids(hp, lens, 95)
    d_t, d_cu, d_out = hip.upload(toks), hip.upload(cu), hip.nans((B, H))
    out = [(d_out, (B, H), np.float32)]
    s, s2 = hip.stream(), hip.stream()
    call = lambda stream: m.lib.bert_hip_eval_packed_device(m.ctx, d_t, d_cu, B, T, max(lens), d_out, stream)
    with hip.capture(s) as cap:
        r = call(s)
    err = capfd.readouterr().err
    seen = f"the call returned {r} ({err.strip()!r}), hipStreamEndCapture {cap.status}, graph {cap.graph}, capture status afterwards {hip.capture_status(s)}"
    print("allocation under capture:", seen)
    assert r != 0 and "bert_hip_eval_packed_device" in err, seen
    assert cap.status != OK and not cap.graph, "a call that failed must not leave a launchable graph: " + seen
    assert np.isnan(hip.download(d_out, (B, H))).all()
    hip.destroy_stream(s)
    # the context is as good as before
    want = m.eval_packed(toks, cu)
    for stream in (s2, 0):
        (got,) = _eager(hip, lambda: call(stream), out)
        assert m.check() == 0 and _same(got, want), (stream, seen)
    graph, ex = _captured(hip, s2, lambda: call(s2), out)
    _all_same(_replay(hip, ex, s2, out), [want], "a clean capture afterwards")
    hip.destroy(ex, graph)
    hip.destroy_stream(s2)
    hip.free(d_t, d_cu, d_out)
    m.close()
