"""Long texts without a GPU: the window plan (bert_hip_plan_windows) against its Python restatement, the untruncated tokenization
(bert_hip_tokenize_long) on a tokenizer-only context, and the grouped pooling's derived error bound (long_text_reference.py) held
against an emulation of the kernel's arithmetic — and against two wrong kernels, which must leave it."""
import ctypes as C

import numpy as np
import pytest

import long_text_reference as ltr
from bert_cpp_amd import pybert

I32P = C.POINTER(C.c_int32)


def c_plan(n_tokens, window, stride, cap=None):
    """(return value, starts written) of bert_hip_plan_windows into a buffer of cap entries (None: as many as it asks for) pre-filled with -7"""
    L = pybert.lib()
    n = L.bert_hip_plan_windows(n_tokens, window, stride, None, 0)
    if n < 0 or cap == 0:
        return n, []
    buf = np.full(max(n, cap or 0) + 2, -7, dtype=np.int32)
    r = L.bert_hip_plan_windows(n_tokens, window, stride, buf.ctypes.data_as(I32P), n if cap is None else cap)
    return r, buf.tolist()


def test_plan_windows_equals_the_restatement_and_has_its_properties():
    checked = total = 0
    for window in range(3, 15):
        c = window - 2
        for stride in range(1, c + 1):
            for n in range(2, 61):
                want = ltr.plan_windows(n, window, stride)
                r, buf = c_plan(n, window, stride)
                total += 1
                assert r == len(want) and buf[:r] == want and buf[r:] == [-7] * (len(buf) - r), (n, window, stride)
                m = n - 2
                if n <= window:
                    assert want == [0]                                      # one window: the text itself
                    continue
                assert r == 1 + -(-(m - c) // stride)                       # the count formula
                assert want[0] == 0 and want[-1] + c == m                   # starts at the text's start, ends at its end
                assert all(0 <= s and s + c <= m for s in want)             # every window has exactly `window` ids of the text
                assert all(b - a == stride for a, b in zip(want[:-2], want[1:-1])) and 0 < want[-1] - want[-2] <= stride
                covered = np.zeros(m, bool)
                for s in want:
                    covered[s:s + c] = True
                assert covered.all()                                        # every inner id is in at least one window
                checked += 1
    assert total == 78 * 59 and checked == 3874                            # (every legal stride of every window; the long texts among them)


@pytest.mark.parametrize("args", [(1, 8, 3), (0, 8, 3), (-5, 8, 3), (20, 2, 1), (20, 0, 1), (20, 8, 0), (20, 8, -1), (20, 8, 7), (20, 3, 2)])
def test_plan_windows_refuses_illegal_arguments(args):
    assert ltr.plan_windows(*args) is None
    buf = np.full(64, -7, dtype=np.int32)
    assert pybert.lib().bert_hip_plan_windows(*args, buf.ctypes.data_as(I32P), 64) == -2
    assert (buf == -7).all()
    with pytest.raises(ValueError):
        pybert.plan_windows(*args)


def test_plan_windows_cap():
    want = ltr.plan_windows(60, 8, 3)
    n = len(want)
    assert n == 19                                                          # 1 + ceil((58 - 6) / 3)
    for cap in (0, 1, n - 1):                                               # too small: the count, nothing written
        r, buf = c_plan(60, 8, 3, cap)
        assert r == n and all(v == -7 for v in buf)
    for cap in (n, n + 2):
        r, buf = c_plan(60, 8, 3, cap)
        assert r == n and buf[:n] == want and all(v == -7 for v in buf[n:])
    assert pybert.lib().bert_hip_plan_windows(60, 8, 3, None, 100) == n      # (no buffer: a count)
    assert c_plan(5, 8, 3, 1) == (1, [0, -7, -7]) and c_plan(5, 8, 3, 0) == (1, [])
    assert pybert.plan_windows(60, 8, 3) == want


def test_windows_of_a_text(sparse_vocab_model):
    ids = [101] + list(range(1000, 1020)) + [102]
    ws = ltr.windows_of(ids, 8, 4)
    assert ws[0] == [101] + list(range(1000, 1006)) + [102] and ws[-1] == [101] + list(range(1014, 1020)) + [102]
    assert all(len(w) == 8 for w in ws) and len(ws) == len(ltr.plan_windows(22, 8, 4))
    assert ltr.windows_of(ids, 22, 4) == [ids] and ltr.windows_of(ids, 30, 1) == [ids]
    toks, cu, gcu = ltr.pack_groups([ws, [ids]])
    assert cu.tolist() == [8 * i for i in range(len(ws) + 1)] + [8 * len(ws) + 22] and gcu.tolist() == [0, len(ws), len(ws) + 1]
    assert toks[:8].tolist() == ws[0] and toks[-22:].tolist() == ids


def test_tokenize_long(sparse_vocab_model, tok_golden):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        # texts that fit: bert_tokenize's ids
        for t in tok_golden["tests"]:
            text = t["text"] if isinstance(t, dict) else t[0]
            assert m.tokenize_long(text) == m.tokenize(text), text
        assert m.tokenize_long("") == [101, 102]
        # several hundred known words, beyond the 512 ids the truncating call keeps
        words = [p for p in tok_golden["sparse_vocab"].values() if p.isascii() and p.isalpha() and p.islower()]
        inner = {w: m.tokenize(w)[1:-1] for w in words}
        words = [w for w in words if inner[w]]
        assert len(words) > 20
        rng = np.random.default_rng(5)
        seq = [words[i] for i in rng.integers(0, len(words), 700)]
        text = " ".join(seq)
        ids = m.tokenize_long(text)
        assert len(ids) > 512 and ids[0] == 101 and ids[-1] == 102
        assert ids[1:-1] == [i for w in seq for i in inner[w]]
        cut = m.tokenize(text)
        assert len(cut) == 512 and cut[-1] == 102 and ids[:511] == cut[:511]
        # a cap that is too small: the count, nothing written
        n = len(ids)
        buf = np.full(n + 3, -7, dtype=np.int32)
        assert m.lib.bert_hip_tokenize_long(m.ctx, text.encode(), buf.ctypes.data_as(I32P), n - 1) == n and (buf == -7).all()
        assert m.lib.bert_hip_tokenize_long(m.ctx, text.encode(), None, 0) == n
        assert m.lib.bert_hip_tokenize_long(m.ctx, text.encode(), buf.ctypes.data_as(I32P), n) == n
        assert buf[:n].tolist() == ids and (buf[n:] == -7).all()
        # the text entry points need a device
        out = np.zeros(4, np.float32)
        rows = (C.POINTER(C.c_float) * 1)(out.ctypes.data_as(C.POINTER(C.c_float)))
        txt = (C.c_char_p * 1)(b"a b")
        assert m.lib.bert_hip_encode_long_batch(m.ctx, 1, 1, txt, 8, 3, rows, None) == -1
        assert m.lib.bert_hip_index_add_long_texts(None, 1, 1, txt, 8, 3) == -1
        assert (out == 0).all()
    finally:
        m.close()


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("H", ltr.KERNEL_WIDTHS)
def test_the_bound_holds_the_kernels_arithmetic_and_not_two_wrong_ones(H, raw):
    rows, weights, group_cu = ltr.kernel_case(H)
    want = ltr.group_pool(rows, weights, group_cu, raw)
    bound = ltr.group_pool_bound(rows, weights, group_cu, raw)
    got = ltr.group_pool_f32(rows, weights, group_cu, raw)
    assert np.isfinite(got).all() and np.isfinite(bound).all() and (bound >= 0).all()
    frac = np.abs(got - want) / np.where(bound > 0, bound, 1)
    assert (np.abs(got - want) <= bound).all(), float(frac.max())
    sizes = np.diff(group_cu)
    if raw:                                                                 # a group of one sentence is its row
        assert (bound[sizes == 1] == 0).all() and np.array_equal(got[sizes == 1], rows[group_cu[:-1][sizes == 1]])
    many = sizes > 1
    for wrong in ({"drop_last": True}, {"unit_weights": True}):
        bad = ltr.group_pool_f32(rows, weights, group_cu, raw, **wrong)
        assert np.array_equal(bad[~many], got[~many])                       # (neither touches a group of one)
        if H == 1 and not raw:
            continue                                                        # (a normalised row of one element is +-1 whatever the weights)
        for g in np.nonzero(many)[0]:
            assert (np.abs(bad[g] - want[g]) > bound[g]).any(), (wrong, int(g))
    # unit weights where they are due: the same bound with w = 1
    want1 = ltr.group_pool(rows, None, group_cu, raw)
    got1 = ltr.group_pool_f32(rows, None, group_cu, raw)
    assert (np.abs(got1 - want1) <= ltr.group_pool_bound(rows, None, group_cu, raw)).all()
