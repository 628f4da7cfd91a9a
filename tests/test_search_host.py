"""Embedding index (bert_hip_index_*, include/bert_hip.h) without a GPU: the contexts and programs that cannot hold an
index say so and fail."""
import os
import subprocess

from bert_cpp_amd import pybert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")


def test_index_on_a_tokenizer_only_context_is_refused(sparse_vocab_model, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        capfd.readouterr()
        assert not m.lib.bert_hip_index_create(m.ctx, 0, 1)
        assert "bert_hip_index_create" in capfd.readouterr().err
        try:
            m.index()
        except RuntimeError as e:
            assert "bert_hip_index_create" in str(e)
        else:
            raise AssertionError("BertModel.index() on a tokenizer-only context did not raise")
        # the other entry points refuse a missing index instead of crashing
        assert m.lib.bert_hip_index_size(None) == -1
        assert m.lib.bert_hip_index_add(None, 0, None) < 0
        m.lib.bert_hip_index_free(None)
    finally:
        m.close()


def _search_tool():
    subprocess.run(["make", "-C", os.path.join(ROOT, "bert.cpp_amd"), "examples"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(BIN, "bert-search")


def test_search_example_fails_loudly_without_a_device_or_model(make_model, tmp_path):
    import torch
    exe = _search_tool()
    texts = tmp_path / "texts.txt"
    texts.write_text("one\ntwo\n")
    r = subprocess.run([exe, "-m", "/nonexistent/model.bin", "-f", str(texts)], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "failed to load model" in r.stderr
    if not torch.cuda.is_available():
        path, _ = make_model("tiny", "f16", 0)
        r = subprocess.run([exe, "-m", path, "-f", str(texts)], input="q\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "failed to load model" in r.stderr
