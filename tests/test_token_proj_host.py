"""The projection head's host side, no GPU: names, the loader's limits on P, the converter, and that the derived bound can be met."""
import os, re, subprocess
import numpy as np
import pytest
from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert
from conftest import ROOT
from maxsim_reference import chain_f32
import token_proj_reference as tp

def test_the_name_and_the_hook_are_declared_listed_and_exported():
    assert "bert_hip_token_dim" in pybert.BERT_HIP_H_SYMBOLS and "bert_hip_test_token_project" in pybert.BERT_HIP_TEST_H_SYMBOLS
    declared = lambda hdr: set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", open(os.path.join(ROOT, "include", hdr)).read()))
    assert "bert_hip_token_dim" in declared("bert_hip.h") and "bert_hip_test_token_project" in declared("bert_hip_test.h")
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.split()
    product, hooks = nm(pybert.LIB_PATH), nm(pybert.TEST_LIB_PATH)
    assert "bert_hip_token_dim" in product and "bert_hip_token_dim" in hooks
    assert "bert_hip_test_token_project" in hooks and "bert_hip_test_token_project" not in product
    assert pybert.lib().bert_hip_token_dim(None) == -1

@pytest.mark.parametrize("P,refused", [(48, True), (288, True), (0, False)])
def test_loader_refuses_other_dims_and_a_tokenizer_ignores_the_head(tmp_path, capfd, P, refused):
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 0)
    w[gf.TOKEN_PROJ_NAME] = np.ones((P or 96, hp.n_embd), np.float32)
    path = str(tmp_path / "m.bin")
    gf.write_model(path, hp, w, gf.FTYPE_Q4_0)
    assert gf.read_model(path).raw[gf.TOKEN_PROJ_NAME][0] == gf.FTYPE_F16          # never q4
    if refused:
        assert not pybert.lib().bert_load_from_file(path.encode())
        err = capfd.readouterr().err
        assert f"a projection to {P} dims" in err and "multiple of 32 from 32 to 256" in err
    m = pybert.BertModel(path, tokenizer_only=True)
    assert m.token_dim == 0
    m.close()

def test_hf_colbert_weights_round_trip(tmp_path):
    hp = gf.MODEL_DIMS["tiny"]
    w = gf.synthetic_weights(hp, 3)
    w[gf.TOKEN_PROJ_NAME] = np.random.default_rng(3).normal(0, 0.1, (64, hp.n_embd)).astype(np.float32)
    sd = {"bert." + k: v for k, v in w.items() if k != gf.TOKEN_PROJ_NAME}
    sd.update({"linear.weight": w[gf.TOKEN_PROJ_NAME], "bert.embeddings.position_ids": np.arange(hp.n_max_tokens),
               "bert.pooler.dense.weight": np.zeros((hp.n_embd, hp.n_embd), np.float32)})
    got = gf.hf_colbert_weights(sd)
    assert set(got) == set(w) and all(np.array_equal(got[k], w[k]) for k in w)
    gf.write_model(str(tmp_path / "colbert.bin"), hp, got, gf.FTYPE_F32)
    assert np.array_equal(gf.read_model(str(tmp_path / "colbert.bin")).dequantized(gf.TOKEN_PROJ_NAME), w[gf.TOKEN_PROJ_NAME])

@pytest.mark.parametrize("T,H,P", [(33, 40, 96), (5, 384, 256)])
def test_the_derived_bound_can_be_met(T, H, P):
    rng = np.random.default_rng(H)
    x, wp = rng.normal(0.1, 1, (T, H)).astype(np.float16), rng.normal(0, 1 / np.sqrt(H), (P, H)).astype(np.float16)
    v = chain_f32(x, wp)
    for normalize in (False, True):
        for f16_out in (False, True):
            got = tp.normalize_f32(v) if normalize else v
            got = got.astype(np.float16) if f16_out else got
            want, bound = tp.project_reference(x, wp, normalize, f16_out)
            assert np.isfinite(bound).all() and (np.abs(got.astype(np.float64) - want) <= bound).all()
    xi, wi = tp.exact_operands(rng, T, H, P)                  # exact sums: the restated chain is float64's
    assert np.array_equal(chain_f32(xi, wi), (xi.astype(np.float64) @ wi.astype(np.float64).T).astype(np.float32))
