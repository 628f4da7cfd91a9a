"""bench.py's own contract: a plain run prints the headline line and nothing it does not need; --dump-outputs writes what
the timed path computed in its last step."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def test_dump_outputs_float32_and_seeded_sample(tmp_path):
    bench = load_bench()
    small = np.random.default_rng(1).standard_normal((256, 384)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"embeddings": small})
    got = np.load(tmp_path / "a" / "embeddings.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    # above the limit: a fixed seeded sample of rows, the same rows every time, and the files stay under the limit
    big = np.lib.stride_tricks.as_strided(np.arange(768, dtype=np.float32), shape=(bench.DUMP_LIMIT // (768 * 4) + 10, 768),
                                          strides=(0, 4))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"embeddings": big})
        assert not (tmp_path / d / "embeddings.npy").exists()
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= bench.DUMP_LIMIT
    rows_b = np.load(tmp_path / "b" / "embeddings_sample_rows.npy")
    assert rows_b.dtype == np.float64 and len(rows_b) == bench.DUMP_SAMPLE_ROWS and np.all(np.diff(rows_b) > 0)
    assert np.array_equal(rows_b, np.load(tmp_path / "c" / "embeddings_sample_rows.npy"))
    sample = np.load(tmp_path / "b" / "embeddings_sample.npy")
    assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_SAMPLE_ROWS, 768)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run times exactly --steps steps in one region, prints the contract keys, and its dump holds the embeddings the
    same batch gets through the host API."""
    env = dict(os.environ, BERT_HIP_QUIET="1")
    env.pop("BERT_HIP_LATENCY", None)
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2 and line["regions"]["n"] == 1 and line["regions"]["steps_each"] == 7
    assert line["unit"] == "sentences/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert abs(line["value"] - 256 * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    assert "roofline" not in line and "also" not in line and "cpu_baseline" not in line
    assert not (tmp_path / "bench_detail.json").exists()
    got = np.load(out_dir / "embeddings.npy")
    assert got.dtype == np.float32 and got.shape == (256, 384)

    bench = load_bench()
    from bert_cpp_amd import ggml_file as gf
    from bert_cpp_amd import pybert
    cfg = bench.CONFIGS[1]
    hp = gf.MODEL_DIMS[cfg["dims"]]
    path = str(tmp_path / "m.bin")
    gf.make_synthetic_model(path, cfg["dims"], cfg["ftype"], seed=0)
    flat, cu, _ = bench.config_inputs(cfg, 1, hp, 0)
    m = pybert.BertModel(path)
    want = m.eval_packed(flat, cu)
    m.close()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
