"""Host logic of the API layer (csrc/context.cpp, gather.cpp, text_batch.cpp) through the test library, each against a Python
restatement — no GPU needed: the BERT_HIP_DEVICES parser, the super-batch cut of the gather, the group schedule of
bert_encode_batch and the tokenize + validate + pack step the text entry points share."""
import random

import numpy as np

from bert_cpp_amd import pybert

from conftest import write_vocab_only_model


# ------------------------------------------------------------------------------------------------ device list
def _strtol(s, i):
    """C strtol(s + i, &end, 10) -> (value, end); end == i: nothing converted."""
    j = i
    while j < len(s) and s[j] in " \t\n\v\f\r":
        j += 1
    neg = j < len(s) and s[j] == "-"
    if j < len(s) and s[j] in "+-":
        j += 1
    k = j
    while k < len(s) and s[k] in "0123456789":
        k += 1
    return (0, i) if k == j else (-int(s[j:k]) if neg else int(s[j:k]), k)


def _parse_devices(spec, n_devices, current):
    if not spec:
        return [current if 0 <= current < n_devices else 0], None
    devs, p = list(range(n_devices)) if spec == "all" else [], 0
    while spec != "all" and p < len(spec):
        d, end = _strtol(spec, p)
        if end == p:
            return None, f"BERT_HIP_DEVICES: cannot parse '{spec}'"
        if not 0 <= d < n_devices:
            return None, f"BERT_HIP_DEVICES: ordinal {d} out of range"
        devs.append(d)
        p = end + 1 if spec[end:end + 1] == "," else end
    if not devs:
        return None, "BERT_HIP_DEVICES names no device"
    for i, d in enumerate(devs):
        if d in devs[:i]:
            return None, f"BERT_HIP_DEVICES lists device {d} twice"
    return devs, None


def test_device_list_table():
    """What BERT_HIP_DEVICES (or its alias BERT_HIP_DEVICE) may hold, on a box of 8 devices with device 3 current."""
    table = {
        "": ([3], None), "all": (list(range(8)), None), "0": ([0], None), "3,1": ([3, 1], None),
        "1,": ([1], None),                                                     # a trailing comma is accepted
        "1,,2": (None, "BERT_HIP_DEVICES: cannot parse '1,,2'"),               # an empty element is not
        "1x": (None, "BERT_HIP_DEVICES: cannot parse '1x'"),                   # nor is trailing garbage
        "-1": (None, "BERT_HIP_DEVICES: ordinal -1 out of range"),
        "8": (None, "BERT_HIP_DEVICES: ordinal 8 out of range"),
        "2,2": (None, "BERT_HIP_DEVICES lists device 2 twice"),
    }
    for spec, want in table.items():
        assert pybert.parse_devices(spec.encode(), 8, 3) == want, spec
        assert _parse_devices(spec, 8, 3) == want, spec
    assert pybert.parse_devices(None, 8, 3) == ([3], None)                     # unset: the caller's current device
    assert pybert.parse_devices(None, 2, 5) == ([0], None)                     # (a current device the count does not cover)
    assert pybert.parse_devices(b"7", 8, 3) == ([7], None)
    assert pybert.parse_devices(b"all", 1, 0) == ([0], None)


def test_device_list_random_against_restatement():
    rnd = random.Random(5)
    pieces = [str(i) for i in range(10)] + ["10", "63", ",", ",", ",", "x", "-1", "-", "+2", " ", "all", "a"]
    seen = set()
    for _ in range(600):
        spec = "".join(rnd.choice(pieces) for _ in range(rnd.randint(0, 6)))
        n_devices, current = rnd.randint(1, 8), rnd.randint(0, 8)
        want = _parse_devices(spec, n_devices, current)
        assert pybert.parse_devices(spec.encode(), n_devices, current) == want, (spec, n_devices, current)
        seen.add("a list" if want[1] is None else next(k for k in ("cannot parse", "out of range", "twice") if k in want[1]))
    assert seen == {"a list", "cannot parse", "out of range", "twice"}


# ------------------------------------------------------------------------------------------------ gather runs
def _cu(lens, first=0):
    return (first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)


def _gather_runs(cu, tokens_per_run):
    n, runs = len(cu) - 1, [0]
    for b in range(1, n + 1):
        if b == n or int(cu[b + 1]) - int(cu[runs[-1]]) > tokens_per_run:
            runs.append(b)
    return runs


def test_gather_runs_against_restatement_and_properties():
    rng = np.random.default_rng(2)
    cases = [([128] * 1000, 4096), ([128] * 1000, 128), ([128] * 1000, 127), ([7], 100), ([7], 3), ([512, 1, 1, 512, 3], 100),
             ([3, 400, 2, 2, 400, 400, 1], 64)]                                # (sentences longer than a run)
    for _ in range(200):
        n = int(rng.integers(1, 400))
        lens = rng.integers(1, 513, n) if rng.integers(2) else np.clip(np.round(rng.lognormal(np.log(21.0), 0.7, n)), 1, 128).astype(int)
        cases.append((lens.tolist(), int(rng.choice([1, 100, 512, 513, 3000, 10000, 10 ** 6, 4 * 262144 * 8]))))
    for lens, per_run in cases:
        cu = _cu(lens, first=int(rng.integers(0, 2)) * 1000)                  # (the cut depends on differences only)
        runs = pybert.gather_runs(cu, per_run)
        assert runs == _gather_runs(cu, per_run), (lens[:8], per_run)
        n = len(lens)
        assert runs[0] == 0 and runs[-1] == n and all(a < b for a, b in zip(runs, runs[1:]))
        for a, b in zip(runs, runs[1:]):
            assert int(cu[b]) - int(cu[a]) <= per_run or b - a == 1            # only a single sentence exceeds a run
            if b < n:
                assert int(cu[b + 1]) - int(cu[a]) > per_run                   # the run could not have taken the next sentence
    assert pybert.gather_runs(_cu([128] * 1024), 128 * 256) == [0, 256, 512, 768, 1024]


# ------------------------------------------------------------------------------------------------ group schedule
def test_encode_group_schedule():
    rnd = random.Random(9)
    ns = list(range(1, 40)) + [2047, 2048, 2049, 2559, 2560, 2561, 6143, 6144, 6655, 6656, 7168, 14335, 14336, 16383, 16384, 30720,
                               32768, 34815, 34816, 10 ** 5, 10 ** 6] + [rnd.randint(1, 10 ** 6) for _ in range(300)]
    for n in ns:
        groups = pybert.encode_groups(n)
        assert sum(groups) == n and all(g > 0 for g in groups), n
        left = n
        for k, g in enumerate(groups):
            size = 2048 << min(k, 3)                                           # 2048, 4096, 8192, then 16384
            if k + 1 < len(groups):
                assert g == size and left - g >= size // 4, (n, k)             # what stays behind is a quarter of it or more
            else:
                assert g == left < size + size // 4, (n, k)                    # the last one absorbs less than a quarter
            left -= g
    assert pybert.encode_groups(0) == []
    assert pybert.encode_groups(2559) == [2559] and pybert.encode_groups(2560) == [2048, 512]
    assert pybert.encode_groups(32768) == [2048, 4096, 8192, 18432] and pybert.encode_groups(34816) == [2048, 4096, 8192, 16384, 4096]
    assert pybert.encode_groups(10 ** 5)[:5] == [2048, 4096, 8192, 16384, 16384]


# ------------------------------------------------------------------------------------------------ tokenize + pack
WORDS = ("the of and to in a is that for it as was with be by on not he this are or his from at which but have an had they you "
         "were their one all we can her has there been if more when will would who so no embedding tokenizer sentence").split()


def _vocab_model(tmp_path_factory, n_max_tokens):
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(1, 100)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += list("abcdefghijklmnopqrstuvwxyz0123456789.,!?") + WORDS + ["##s", "##ing", "##ed", "##ly", "##a", "##e", "##n", "##t"]
    path = str(tmp_path_factory.mktemp("api_host") / f"vocab_{n_max_tokens}.bin")
    write_vocab_only_model(path, vocab, n_max_tokens=n_max_tokens)
    return path


def _texts(seed, n, max_words):
    rnd = random.Random(seed)
    return [" ".join(rnd.choice(WORDS) + rnd.choice(["", "", "s", "ing", "ed", ".", "!"]) for _ in range(rnd.randint(0, max_words))).encode()
            for _ in range(n)]


def _concat(rows):
    return [t for r in rows for t in r]


def test_tokenize_pack_equals_the_batch_tokenizer_rows_concatenated(tmp_path_factory):
    """One TokenGroup serves bert_encode_batch and the index's *_texts entries: counts, prefix sums and the ids back to back are
    bert_hip_tokenize_batch's rows concatenated, on 1, 2 and 16 threads, and a smaller batch on the same (grow-only, never
    cleared) group leaves nothing of the larger one behind."""
    m = pybert.BertModel(_vocab_model(tmp_path_factory, 64), tokenizer_only=True, test_routes=True)
    big, small = _texts(1, 700, 30), _texts(2, 50, 12)
    for texts in (big, small, big[:1], []):
        rows = m.tokenize_batch(texts, 4)
        assert all(2 <= len(r) <= 64 for r in rows)
        for n_threads in (1, 2, 16):
            n_ok, counts, cu, packed = pybert.tokenize_pack(m, texts, n_threads)
            assert n_ok == len(texts) and counts == [len(r) for r in rows]
            assert cu == _cu([len(r) for r in rows]).tolist() and packed == _concat(rows), (len(texts), n_threads)
    # n_max_tokens so small that most texts are cut: the tokenizer truncates, every text can still be evaluated
    m16 = pybert.BertModel(_vocab_model(tmp_path_factory, 16), tokenizer_only=True, test_routes=True)
    rows = m16.tokenize_batch(big, 4)
    assert sum(len(r) == 16 for r in rows) > 300
    n_ok, counts, cu, packed = pybert.tokenize_pack(m16, big, 16)
    assert n_ok == len(big) and max(counts) == 16 and cu[-1] == sum(counts) and packed == _concat(rows)


def test_pack_stops_in_front_of_the_first_text_that_cannot_be_evaluated(tmp_path_factory):
    """A text cannot be evaluated if its token count is outside 1 .. n_max_tokens.  No text produces such a count — the tokenizer
    always emits [CLS] and [SEP] and truncates at n_max_tokens — so the rule is exercised on the pack step with counts supplied
    in place of the tokenizer's: everything in front of the first bad count is packed, nothing behind it."""
    m = pybert.BertModel(_vocab_model(tmp_path_factory, 64), tokenizer_only=True, test_routes=True)
    texts = _texts(3, 200, 30)
    rows = m.tokenize_batch(texts, 4)
    true = [len(r) for r in rows]
    for bad_at, bad in ((0, 0), (5, 0), (120, -3), (199, 65), (37, 1000)):
        counts = list(true)
        counts[bad_at] = bad
        counts[(bad_at + 50) % 200] = 65 if bad <= 0 else 0                    # (a later bad one changes nothing)
        first = min(bad_at, (bad_at + 50) % 200)
        n_ok, got, cu, packed = pybert.tokenize_pack(m, texts, 2, counts=counts)
        assert n_ok == first and got == counts
        assert cu == _cu(true[:first]).tolist() and packed == _concat(rows[:first])
    # the bounds themselves are fine: 1 token, and counts no larger than the text's own
    counts = [1 if i % 3 == 0 else c for i, c in enumerate(true)]
    n_ok, _, cu, packed = pybert.tokenize_pack(m, texts, 2, counts=counts)
    assert n_ok == 200 and cu == _cu(counts).tolist() and packed == _concat(r[:c] for r, c in zip(rows, counts))
