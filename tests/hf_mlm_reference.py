"""The HuggingFace side of tests/test_sparse_host.py::test_float64_model_matches_huggingface, in a process of its own (as
hf_cross_encoder_reference.py).  Test infrastructure only.

usage: python hf_mlm_reference.py <dims> <out_dir>  ->  <out_dir>/hf_mlm_<dims>.bin (an f32 model file with an MLM head) and
<out_dir>/hf_mlm.npz (ids<i>, want<i>: sentences and their logits [n, V] from transformers.BertForMaskedLM in float64).  exit code 77:
torch / transformers are not importable."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(dims, out_dir):
    try:
        import torch
        import transformers
    except Exception:
        return 77
    from bert_cpp_amd import ggml_file as gf
    hp = gf.MODEL_DIMS[dims]
    torch.manual_seed(4321)
    cfg = transformers.BertConfig(vocab_size=hp.n_vocab, hidden_size=hp.n_embd, num_hidden_layers=hp.n_layer, num_attention_heads=hp.n_head,
                                  intermediate_size=hp.n_intermediate, max_position_embeddings=hp.n_max_tokens, hidden_act="gelu_new",
                                  layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, type_vocab_size=2,
                                  tie_word_embeddings=True)
    model = transformers.BertForMaskedLM(cfg).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in model.named_parameters():       # (HF's N(0, 0.02) init scaled up: attention and GELU away from their linear range)
            if p.ndim == 2 and "embeddings" not in name:
                p.mul_(2.5)
            elif p.ndim == 2:
                p.mul_(20.0)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    sd = model.state_dict()
    assert sd["cls.predictions.decoder.weight"].data_ptr() == sd["bert.embeddings.word_embeddings.weight"].data_ptr(), "the decoder is not tied"
    assert torch.equal(sd["cls.predictions.decoder.bias"], sd["cls.predictions.bias"])
    path = os.path.join(out_dir, f"hf_mlm_{dims}.bin")
    gf.write_model(path, hp, gf.hf_mlm_weights(sd, hp.n_layer), gf.FTYPE_F32)
    model = model.double()
    rng = np.random.default_rng(5)
    out = {"n": np.int64(0)}
    for i, total in enumerate([1, 3, 37, 64]):
        ids = rng.integers(1, hp.n_vocab, size=total).astype(np.int32)
        with torch.no_grad():
            z = model(input_ids=torch.tensor(ids[None].astype(np.int64))).logits[0]
        out[f"ids{i}"], out[f"want{i}"] = ids, z.numpy().astype(np.float64)
        out["n"] = np.int64(i + 1)
    np.savez(os.path.join(out_dir, "hf_mlm.npz"), **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
