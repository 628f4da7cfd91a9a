"""Long texts on the GPU (include/bert_hip.h "LONG TEXTS"): the grouped-pooling kernel through bert_hip_test_group_pool against
float64 within the derived bound of long_text_reference.py; bert_hip_eval_packed_grouped end to end on three routes in all four
pooling modes; the text entry points (bert_hip_encode_long_batch, bert_hip_index_add_long_texts) against windows built in Python and
against the CPU oracle; bin/bert-search --long."""
import os
import subprocess

import numpy as np
import pytest

import long_text_reference as ltr
from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from oracle import oracle as orc

from conftest import ROOT, cosine
from test_gpu_parity import MIN_COS
from test_gpu_pooling import MODES, _Hip, _cu, _set_mode

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
_WORST = {}


def _hold(got, want, bound, what):
    """|got - want| <= bound everywhere; prints (and records) the worst fraction of the bound"""
    err = np.abs(got.astype(np.float64) - want)
    frac = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    _WORST[what] = max(_WORST.get(what, 0.0), frac)
    print(f"{what}: worst fraction of the bound {frac:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, frac)
    return frac


# ------------------------------------------------------------------------------------------------
# the kernel, through bert_hip_test_group_pool
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", ltr.KERNEL_WIDTHS)
def test_group_pool_kernel_against_float64(H):
    """Group sizes [1, 1, 2, 3, 7, 33] in one call, weights 1 .. 512, rows normal(0.1, 1); NaN rows in front of and behind the rows
    in use, the output buffer NaN beforehand: every word finite afterwards, both forms within the bound."""
    rows, weights, gcu = ltr.kernel_case(H)
    assert np.isnan(rows[:2]).all() and np.isnan(rows[-2:]).all()
    for raw in (True, False):
        for w in (weights, None):
            got, st = pybert.test_group_pool(rows, w, gcu, raw, np.full((len(gcu) - 1, H), np.nan, dtype=np.float32))
            assert st == 0
            _hold(got, ltr.group_pool(rows, w, gcu, raw), ltr.group_pool_bound(rows, w, gcu, raw),
                  f"kernel H {H} {'raw' if raw else 'normalised'} {'token' if w is not None else 'unit'} weights")
            if raw:                                                         # a group of one sentence: its row, unchanged
                assert np.array_equal(got[0], rows[gcu[0]]) and np.array_equal(got[1], rows[gcu[1]])


@pytest.mark.parametrize("H", ltr.KERNEL_WIDTHS)
def test_a_groups_bits_depend_on_its_own_rows_only(H):
    rows, weights, gcu = ltr.kernel_case(H)
    G = len(gcu) - 1
    for raw in (True, False):
        got, _ = pybert.test_group_pool(rows, weights, gcu, raw)
        # alone
        for g in range(G):
            s0, s1 = int(gcu[g]), int(gcu[g + 1])
            alone, st = pybert.test_group_pool(rows[s0:s1], weights[s0:s1], [0, s1 - s0], raw)
            assert st == 0 and np.array_equal(alone[0], got[g]), (H, raw, g)
        # in another position, among the same groups in reverse order (no NaN rows around them this time)
        order = list(range(G))[::-1]
        r2 = np.concatenate([rows[gcu[g]:gcu[g + 1]] for g in order])
        w2 = np.concatenate([weights[gcu[g]:gcu[g + 1]] for g in order])
        rev, st = pybert.test_group_pool(r2, w2, _cu([int(gcu[g + 1] - gcu[g]) for g in order]), raw)
        assert st == 0 and np.array_equal(rev[::-1], got), (H, raw)


def test_group_pool_kernel_guard():
    """An empty group, one that runs backwards and one that leaves the rows: NaN rows and the status word; the neighbours keep their bits."""
    rows, weights, _ = ltr.kernel_case(64)
    rows = rows[2:-2]
    weights = weights[2:-2]
    n = len(rows)
    good, st = pybert.test_group_pool(rows, weights, [0, 3, 10, n], False)
    assert st == 0 and np.isfinite(good).all()
    for bad in ([0, 3, 3, 10, n], [0, 3, 10, 3, n], [0, 3, n + 1, n]):
        got, st = pybert.test_group_pool(rows, weights, bad, False)
        assert st == 1
        assert np.array_equal(got[0], good[0])
        nan = np.isnan(got).all(axis=1)
        assert nan.any() and (nan | np.isfinite(got).all(axis=1)).all()
    got, st = pybert.test_group_pool(rows, weights, [0, 3, 3, 10, n], False)
    assert np.isnan(got).all(axis=1).tolist() == [False, True, False, False]
    assert np.array_equal(got[3], good[2])                                  # rows 10 .. n: the same group as before
    # a NaN row of a sentence makes its group's row NaN, and only that one
    rows2 = rows.copy()
    rows2[5] = np.nan
    got, st = pybert.test_group_pool(rows2, weights, [0, 3, 10, n], True)
    assert st == 0 and np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


@pytest.mark.parametrize("H", [64, 130, 384, 768])
def test_groups_of_one_sentence_are_the_ordinary_poolings_bits(H):
    """test_pool(..., normalize=False)'s rows in, every sentence a group of its own: test_pool(..., normalize=True)'s bits out."""
    rng = np.random.default_rng(H)
    lens = [1, 2, 3, 5, 31, 64, 128]
    cu = _cu(lens)
    x = rng.normal(0.1, 1, (int(cu[-1]), H)).astype(np.float16)
    for pooling in ("mean", "cls"):
        raw, st = pybert.test_pool(x, cu, 128, pooling, False)
        want, st2 = pybert.test_pool(x, cu, 128, pooling, True)
        assert st == 0 and st2 == 0
        w = lens if pooling == "mean" else None
        got, st = pybert.test_group_pool(raw, w, np.arange(len(lens) + 1), False)
        assert st == 0 and np.array_equal(got, want), (H, pooling)
        got, st = pybert.test_group_pool(raw, w, np.arange(len(lens) + 1), True)
        assert st == 0 and np.array_equal(got, raw), (H, pooling)


# ------------------------------------------------------------------------------------------------
# end to end, through bert_hip_eval_packed_grouped
# ------------------------------------------------------------------------------------------------
LENS = [1, 2, 5, 16, 17, 31, 64, 127, 128]
GROUPS = [1, 3, 1, 4]
# arm: (dims, ftype, options, kernels the profile of a grouped call must show)
ARMS = {
    "one_launch": ("minilm-l6", "f16", {"one_launch": "2"}, {"model_kernel", "group_pool"}),
    "fused": ("minilm-l6", "f16", {"one_launch": "0", "latency": "0"}, {"qkv_attention2", "layer_tail", "pool_normalize", "group_pool"}),
    "f32": ("tiny", "f32", {}, {"family:gemm_f32", "pool_normalize", "group_pool"}),
}


@pytest.mark.parametrize("arm", list(ARMS))
def test_eval_packed_grouped(arm, make_model, capfd):
    dims, ftype, options, must = ARMS[arm]
    path, hp = make_model(dims, ftype, 6)
    sents = [gf.synthetic_token_ids(1, min(n, hp.n_max_tokens), hp.n_vocab, seed=100 + i)[0] for i, n in enumerate(LENS)]
    lens = [len(s) for s in sents]
    toks, cu, gcu = np.concatenate(sents).astype(np.int32), _cu(lens), _cu(GROUPS)
    B, G, T, H = len(sents), len(GROUPS), int(cu[-1]), hp.n_embd
    hip = _Hip()
    m = pybert.BertModel(path)
    try:
        for k, v in options.items():
            m.set_option(k, v)
        d_t, d_cu, d_g, d_out = hip.upload(toks), hip.upload(cu), hip.upload(gcu), hip.upload(np.zeros((G, H), np.float32))
        d_bad = hip.upload(np.array([0, 1, 1, 5, 9], np.int32))
        for mode in MODES:
            _set_mode(m, mode)
            ordinary = m.eval_packed(toks, cu)
            # the chain by hand: the raw rows under the same pooling, pooled in float64
            m.set_option("normalize", "0")
            raw_rows = m.eval_packed(toks, cu)
            _set_mode(m, mode)
            w = lens if mode[0] == "mean" else None
            is_raw = mode[1] == "0"
            m.profile(True)
            got = m.eval_packed_grouped(toks, cu, gcu)
            names = set(m.profile_report(families=True))
            m.profile(False)
            assert must <= names, (arm, mode, sorted(names))
            with capfd.disabled():                                          # (the figure is printed, not swallowed with the entry points' stderr lines)
                _hold(got, ltr.group_pool(raw_rows, w, gcu, is_raw), ltr.group_pool_bound(raw_rows, w, gcu, is_raw), f"{arm} {mode}")
            # groups of one: the ordinary call's bits in the context's mode; so is every row when every sentence is its own group
            assert np.array_equal(got[0], ordinary[0]) and np.array_equal(got[2], ordinary[4]), (arm, mode)
            assert np.array_equal(m.eval_packed_grouped(toks, cu, np.arange(B + 1)), ordinary), (arm, mode)
            # the settings and an ordinary call are what they were
            assert (m.pooling(), m.normalize()) == (int(mode[0] == "cls"), int(mode[1]))
            assert np.array_equal(m.eval_packed(toks, cu), ordinary), (arm, mode)
            # the chunks of the host path do not show
            m.set_option("chunk_tokens", "200")
            assert np.array_equal(m.eval_packed_grouped(toks, cu, gcu), got), (arm, mode)
            m.set_option("chunk_tokens", "262144")
            # the device entry: the same bits
            m.eval_packed_grouped_device(d_t, d_cu, B, T, max(lens), d_g, G, d_out, 0)
            assert m.check() == 0
            assert np.array_equal(hip.download(d_out, (G, H)), got), (arm, mode)
            # ... and an empty group there: a NaN row and the status word; its neighbours keep their bits
            capfd.readouterr()
            m.eval_packed_grouped_device(d_t, d_cu, B, T, max(lens), d_bad, G, d_out, 0)
            assert m.check() == 1 and m.check() == 0
            dev = hip.download(d_out, (G, H))
            assert np.isnan(dev[1]).all() and np.array_equal(dev[0], got[0]) and np.array_equal(dev[3], got[3]) and np.isfinite(dev[2]).all()
        # a bad group_cu on the host entry: -2, a message, the output untouched
        for bad in ([0, 1, 1, 5, 9], [1, 2, 4, 5, 9], [0, 1, 4, 5, 8], [0, 4, 1, 5, 9], [0, 1, 4, 5, 10]):
            out = np.full((G, H), 7.0, dtype=np.float32)
            capfd.readouterr()
            with pytest.raises(ValueError):
                m.eval_packed_grouped(toks, cu, np.array(bad, np.int32), out)
            assert (out == 7.0).all() and "group_cu" in capfd.readouterr().err, bad
        hip.free(d_t, d_cu, d_g, d_out, d_bad)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------
# texts
# ------------------------------------------------------------------------------------------------
WORDS = ["[PAD]", "[UNK]"] + [f"w{i}" for i in range(2, 101)] + ["[CLS]", "[SEP]"] + list("abcdefghij") + \
        ["hello", "world", "##ing", "##s", "test", ",", ".", "!", "embed", "##ding", "server", "client", "long", "text", "window", "stride",
         "pool", "index", "search", "row"]
FTYPE = "f16"
PREFIX = " ".join(["a b c d e f g h i j"] * 7)              # 70 ids: more than the 62 inner positions of the model
TAIL_A = " ".join(["long text window stride"] * 60)
TAIL_B = " ".join(["pool index search row"] * 60)


@pytest.fixture(scope="module")
def text_model(tmp_path_factory):
    """the `tiny` dims (64 positions) with a vocabulary of real words"""
    hp = gf.MODEL_DIMS["tiny"]
    vocab = [w.encode() for w in WORDS] + [f"[unused{i}]".encode() for i in range(len(WORDS), hp.n_vocab)]
    path = str(tmp_path_factory.mktemp("long") / f"text_model_{FTYPE}.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 4), gf.FTYPE_BY_NAME[FTYPE], vocab=vocab)
    return path, hp


@pytest.fixture(scope="module")
def model(text_model):
    m = pybert.BertModel(text_model[0])
    yield m
    m.close()


def _about_150_ids(seed):
    rng = np.random.default_rng(seed)
    pool = ["hello", "world", "testing", "tests", "a", "b", "c", ",", ".", "!", "embedding", "server", "client", "long", "text", "window"]
    return " ".join(rng.choice(pool, size=120))


def test_texts_that_fit_are_encode_batchs_bits(model):
    texts = ["hello world!", "testing tests, a b c.", "", "HELLO hello Hello", "a " * 61, "a " * 62]
    assert [len(model.tokenize_long(t)) for t in texts[-2:]] == [63, 64]    # (up to the position limit itself)
    got, nw = model.encode_long_batch(texts, return_windows=True)
    assert nw.tolist() == [1] * len(texts)
    assert np.array_equal(got, model.encode_batch(texts))
    assert np.array_equal(model.encode_long_batch(texts, window=64, stride=1), got)


@pytest.mark.parametrize("window", [64, 32])
def test_a_long_text_is_its_windows_pooled(model, text_model, window):
    text = _about_150_ids(window)
    ids = model.tokenize_long(text)
    assert 125 <= len(ids) <= 200 and len(ids) > 2 * model.n_max_tokens
    o = orc.Oracle(text_model[0])
    c = window - 2
    for stride in (1, c // 2, c):
        got, nw = model.encode_long_batch([text], window, stride, return_windows=True)
        starts = model.plan_windows(len(ids), window, stride)
        assert starts == ltr.plan_windows(len(ids), window, stride) and nw.tolist() == [len(starts)]
        ws = ltr.windows_of(ids, window, stride)
        assert len(ws) == len(starts) and all(len(w) == window for w in ws)
        toks, cu, gcu = ltr.pack_groups([ws])
        assert np.array_equal(got, model.eval_packed_grouped(toks, cu, gcu)), (window, stride)
        # the CPU oracle: every window's last hidden states, pooled over all their tokens in float64
        total = sum(o.eval(w, orc.MODE_PLAIN, want_hidden=True)[1][-1].astype(np.float64).sum(axis=0) for w in ws)
        want = total / sum(len(w) for w in ws)
        cos = cosine(got[0], want / np.linalg.norm(want))
        print(f"window {window} stride {stride}: {len(ws)} windows, cosine {cos:.7f}")
        assert cos >= MIN_COS[FTYPE], (window, stride, cos)
        assert abs(float(np.linalg.norm(got[0])) - 1) < 1e-5


def test_what_lies_behind_the_position_limit_reaches_the_embedding(model):
    """Two texts that share their first n_max_tokens ids and differ behind them: one row for bert_encode_batch — today's behaviour,
    what this feature is about —, two for bert_hip_encode_long_batch."""
    a, b = PREFIX + " " + TAIL_A, PREFIX + " " + TAIL_B
    ia, ib = model.tokenize_long(a), model.tokenize_long(b)
    N = model.n_max_tokens
    assert len(ia) > 4 * N and ia[:N] == ib[:N] and ia[N:] != ib[N:]
    cut = model.encode_batch([a, b])
    assert np.array_equal(cut[0], cut[1])
    got = model.encode_long_batch([a, b])
    cos = cosine(got[0], got[1])
    print(f"cosine of the two long texts' rows: {cos:.4f}")
    # (visibly: ten times the distance the project lets a GPU row lie from the CPU's)
    assert np.isfinite(got).all() and cos < 1 - 10 * (1 - MIN_COS[FTYPE])


def test_short_and_long_texts_in_one_call(model):
    texts = ["hello world!", PREFIX + " " + TAIL_A, "", _about_150_ids(1), "a " * 62, _about_150_ids(2), "testing tests.", PREFIX + " " + TAIL_B]
    for window, stride in ((None, None), (32, 7)):
        got, nw = model.encode_long_batch(texts, window, stride, return_windows=True)
        assert np.isfinite(got).all() and (nw >= 1).all() and nw[1] > 1 and nw[0] == 1
        for i, t in enumerate(texts):
            alone, nw1 = model.encode_long_batch([t], window, stride, return_windows=True)
            assert np.array_equal(alone[0], got[i]) and nw1[0] == nw[i], (window, i)
    # a window or stride outside the limits: -2, outputs untouched
    for window, stride in ((2, 1), (65, 10), (64, 0), (64, 63), (32, 31)):
        with pytest.raises(ValueError):
            model.encode_long_batch(texts, window, stride)


def test_more_windows_than_one_group_holds(model):
    """The texts of a call go to the engine in groups of at most 16384 windows, a text's windows never in two groups: 170 texts of
    about 110 windows each are two groups, and no row shows where the cut fell."""
    texts = [_about_150_ids(100 + i % 7) + " hello" * (i % 3) for i in range(170)]
    got, nw = model.encode_long_batch(texts, 32, 1, n_threads=4, return_windows=True)
    assert np.isfinite(got).all() and int(nw.sum()) > 16384 and int(nw.max()) < 200
    cut = int(np.searchsorted(np.cumsum(nw), 16384, side="right"))          # the first text of the second group
    assert 100 < cut < 169
    for i in (0, cut - 1, cut, cut + 1, 169):
        alone, nw1 = model.encode_long_batch([texts[i]], 32, 1, return_windows=True)
        assert nw1[0] == nw[i] == len(model.plan_windows(len(model.tokenize_long(texts[i])), 32, 1)) and np.array_equal(alone[0], got[i]), i
    for i in range(21, 170):                                                # (the same text, the same row, wherever it stands)
        assert np.array_equal(got[i], got[i - 21]), i


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_index_add_long_texts(model, dtype):
    texts = ["hello world!", PREFIX + " " + TAIL_A, _about_150_ids(3), "a b c", PREFIX + " " + TAIL_B]
    rows = model.encode_long_batch(texts, 64, 31)
    a, b = model.index(dtype=dtype), model.index(dtype=dtype)
    try:
        assert a.add_long_texts(texts[:2], 64, 31) == 0 and a.add_long_texts(texts[2:], 64, 31) == 2
        assert b.add(rows) == 0
        ids = np.arange(len(texts), dtype=np.int32)
        assert len(a) == len(b) == len(texts) and np.array_equal(a.get_rows(ids), b.get_rows(ids))
        with pytest.raises(ValueError):
            a.add_long_texts(texts, 64, 63)                                 # stride > window - 2
        with pytest.raises(ValueError):
            a.add_long_texts(texts, 65, 3)                                  # window > n_max_tokens
        assert len(a) == len(texts) and np.array_equal(a.get_rows(ids), b.get_rows(ids))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------
# the example program
# ------------------------------------------------------------------------------------------------
def test_bert_search_long(text_model, tmp_path):
    """One long line whose words behind the position limit are the query's: --long finds it, the default (lines cut at the limit) puts
    a line that looks like the long line's beginning in front of it."""
    path, _ = text_model
    lines = ["hello world", "testing servers, clients!", PREFIX + " " + TAIL_A, "embedding test.", "pool index search row", "long text",
             "a b c d e f g h i j a b c"]
    query = " ".join(["window stride long text"] * 10)
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    first = {}
    for arm, flags in (("long", ["--long"]), ("long_w32", ["--long", "--window", "32", "--stride", "20"]), ("cut", [])):
        r = subprocess.run([exe, "-m", path, "-f", str(f), "-k", "2"] + flags, input=query + "\nq\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert f"Loaded {len(lines)} lines." in out
        first[arm] = next(l for l in out if l.startswith("1. "))[3:]
    assert first["long"] == lines[2] and first["long_w32"] == lines[2]
    assert first["cut"] != lines[2]
    r = subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60)
    assert "--long" in r.stderr and "cut at the model's position limit" in r.stderr
    r = subprocess.run([exe, "-m", path, "-f", str(f), "--window", "32"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--long" in r.stderr
