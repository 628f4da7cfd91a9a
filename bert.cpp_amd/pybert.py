"""ctypes binding of libbert.so — the same way the reference's Python callers bind it
(reference examples/sample_dylib.py:19-59, benchmarks/run_mteb.py:34-72), plus the bert_hip.h
extensions.  There is no fallback: if the shared library (the HIP extension) is missing or does
not load, importing/constructing fails loudly.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BERT_HIP_LIB") or os.path.join(_HERE, "libbert.so")   # BERT_HIP_LIB: tuning builds

# every symbol include/bert.h and include/bert_hip.h declare
BERT_H_SYMBOLS = [
    "bert_params_parse", "bert_load_from_file", "bert_free", "bert_encode", "bert_encode_batch", "bert_tokenize",
    "bert_eval", "bert_eval_batch", "bert_n_embd", "bert_n_max_tokens", "bert_vocab_id_to_token",
]
BERT_HIP_H_SYMBOLS = [
    "bert_hip_load_tokenizer", "bert_hip_tokenize_batch", "bert_hip_n_layer", "bert_hip_n_head", "bert_hip_n_intermediate", "bert_hip_n_vocab",
    "bert_hip_ftype", "bert_hip_device", "bert_hip_n_devices", "bert_hip_pooling", "bert_hip_normalize", "bert_hip_encode_batch", "bert_hip_eval_packed", "bert_hip_eval_packed_gather",
    "bert_hip_eval_packed_device", "bert_hip_reserve", "bert_hip_check", "bert_hip_eval_hidden",
    "bert_hip_profile_enable", "bert_hip_profile_report", "bert_hip_set_option", "bert_hip_version",
    "bert_hip_index_create", "bert_hip_index_free", "bert_hip_index_size", "bert_hip_index_reserve", "bert_hip_index_add",
    "bert_hip_index_add_device", "bert_hip_index_add_texts", "bert_hip_index_search", "bert_hip_index_search_device",
    "bert_hip_index_search_texts", "bert_hip_index_remove", "bert_hip_index_n_live", "bert_hip_index_search_filtered",
    "bert_hip_index_search_filtered_device", "bert_hip_index_compact", "bert_hip_index_save", "bert_hip_index_load",
    "bert_hip_index_rescore", "bert_hip_index_rescore_device", "bert_hip_index_search_rescored", "bert_hip_index_search_rescored_device",
    "bert_hip_index_get_rows", "bert_hip_index_partition", "bert_hip_index_n_lists", "bert_hip_index_partition_centroids",
    "bert_hip_index_partition_lists", "bert_hip_index_kmeans", "bert_hip_index_search_probed", "bert_hip_index_search_probed_device",
    "bert_hip_index_search_probed_filtered", "bert_hip_index_search_probed_filtered_device", "bert_hip_index_search_rescored_probed",
    "bert_hip_index_search_rescored_probed_device", "bert_hip_index_partition_save", "bert_hip_index_partition_load",
    "bert_hip_eval_packed_grouped", "bert_hip_eval_packed_grouped_device", "bert_hip_tokenize_long", "bert_hip_plan_windows",
    "bert_hip_encode_long_batch", "bert_hip_index_add_long_texts",
    "bert_hip_eval_packed_tokens_device", "bert_hip_eval_packed_tokens", "bert_hip_encode_tokens_batch", "bert_hip_maxsim_device", "bert_hip_maxsim",
    "bert_hip_n_labels", "bert_hip_tokenize_pair", "bert_hip_eval_packed_typed", "bert_hip_eval_packed_typed_device", "bert_hip_score_packed",
    "bert_hip_score_packed_device", "bert_hip_score_pairs",
    "bert_hip_has_mlm_head", "bert_hip_sparse_packed", "bert_hip_sparse_packed_device", "bert_hip_sparse_topk_packed",
    "bert_hip_sparse_topk_packed_device", "bert_hip_encode_sparse_batch",
    "bert_hip_sparse_index_create", "bert_hip_sparse_index_free", "bert_hip_sparse_index_size", "bert_hip_sparse_index_reserve",
    "bert_hip_sparse_index_add", "bert_hip_sparse_index_add_device", "bert_hip_sparse_index_add_texts", "bert_hip_sparse_index_search",
    "bert_hip_sparse_index_search_device", "bert_hip_sparse_index_search_texts", "bert_hip_sparse_index_get_rows",
    "bert_hip_sparse_index_remove", "bert_hip_sparse_index_n_live", "bert_hip_sparse_index_search_filtered",
    "bert_hip_sparse_index_search_filtered_device", "bert_hip_sparse_index_rescore", "bert_hip_sparse_index_rescore_device",
    "bert_hip_sparse_index_compact", "bert_hip_sparse_index_save", "bert_hip_sparse_index_load",
    "bert_hip_sparse_index_invert", "bert_hip_sparse_index_inverted_rows", "bert_hip_sparse_index_search_inverted",
    "bert_hip_sparse_index_search_inverted_device", "bert_hip_sparse_index_search_inverted_texts",
    "bert_hip_hybrid_reserve", "bert_hip_hybrid_search", "bert_hip_hybrid_search_device", "bert_hip_hybrid_search_texts",
    "bert_hip_dense_sparse_search_inverted", "bert_hip_dense_sparse_search_inverted_device", "bert_hip_dense_sparse_search_inverted_texts",
    "bert_hip_token_index_create", "bert_hip_token_index_free", "bert_hip_token_index_size", "bert_hip_token_index_n_tokens",
    "bert_hip_token_index_max_query_tokens", "bert_hip_token_index_reserve", "bert_hip_token_index_add", "bert_hip_token_index_add_device",
    "bert_hip_token_index_add_texts", "bert_hip_token_index_get_doc", "bert_hip_token_index_search", "bert_hip_token_index_search_device",
    "bert_hip_token_index_search_texts", "bert_hip_token_index_rescore", "bert_hip_token_index_rescore_device",
    "bert_hip_late_index_remove", "bert_hip_late_index_n_live", "bert_hip_late_index_n_live_tokens", "bert_hip_late_index_search_filtered",
    "bert_hip_late_index_search_filtered_device", "bert_hip_late_index_compact", "bert_hip_late_index_save", "bert_hip_late_index_load",
    "bert_hip_late_index_create", "bert_hip_late_index_dtype", "bert_hip_late_index_get_codes",
    "bert_hip_relative_attention",
]
# include/bert_hip_test.h: the op-level test hooks, exported by libbert_test.so only
BERT_HIP_TEST_H_SYMBOLS = [
    "bert_hip_test_gemm", "bert_hip_test_gemm_lnfold", "bert_hip_test_attention", "bert_hip_test_qkv_attention",
    "bert_hip_test_layer_tail", "bert_hip_test_skinny_tail", "bert_hip_test_skinny_qkv", "bert_hip_test_shard_bounds", "bert_hip_test_build_windows",
    "bert_hip_test_build_windows_device", "bert_hip_test_max_windows", "bert_hip_test_set_window_slots", "bert_hip_test_set_pad",
    "bert_hip_test_dispatch", "bert_hip_test_shard_threads_created", "bert_hip_test_embed_ln", "bert_hip_test_embed_ln_lanes", "bert_hip_test_pool_normalize",
    "bert_hip_test_pool", "bert_hip_test_layernorm",
    "bert_hip_test_f32_gemm", "bert_hip_test_f32_attention", "bert_hip_test_f32_layernorm", "bert_hip_test_f32_embed_ln", "bert_hip_test_f32_pool",
    "bert_hip_test_model_digest", "bert_hip_test_pack_weight", "bert_hip_test_parse_devices", "bert_hip_test_gather_runs",
    "bert_hip_test_encode_groups", "bert_hip_test_tokenize_pack", "bert_hip_test_index_header",
    "bert_hip_test_build_lists", "bert_hip_test_partition_header", "bert_hip_test_group_pool", "bert_hip_test_token_rows",
    "bert_hip_test_embed_ln_typed", "bert_hip_test_cls_head", "bert_hip_test_sparse_vocab", "bert_hip_test_sparse_topk",
    "bert_hip_test_sparse_vocab_geometry", "bert_hip_test_attention_grid", "bert_hip_test_sparse_scan_geometry",
    "bert_hip_test_sparse_index_header", "bert_hip_test_sparse_index_body",
    "bert_hip_test_sparse_scan_geometry_qb", "bert_hip_test_index_plan", "bert_hip_test_hybrid_chunk", "bert_hip_test_token_index_plan",
    "bert_hip_test_late_index_header", "bert_hip_test_late_index_body",
    "bert_hip_test_attention_bias", "bert_hip_test_f32_attention_bias", "bert_hip_test_rel_bias_table",
    "bert_hip_test_sparse_postings_geometry", "bert_hip_test_sparse_postings_segment",
]
TEST_LIB_PATH = LIB_PATH[:-3] + "_test.so"


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile libbert.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", _HERE, f"-j{jobs}", "-s"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def _declare_product_abi(L):
    """argument / result types of include/bert.h + include/bert_hip.h (libbert.so; libbert_test.so holds the same entry points)"""
    vp, i32, f32p, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.bert_load_from_file.restype = vp; L.bert_load_from_file.argtypes = [C.c_char_p]
    L.bert_hip_load_tokenizer.restype = vp; L.bert_hip_load_tokenizer.argtypes = [C.c_char_p]
    L.bert_free.restype = None; L.bert_free.argtypes = [vp]
    for fn in ("bert_n_embd", "bert_n_max_tokens", "bert_hip_n_layer", "bert_hip_n_head", "bert_hip_n_intermediate",
               "bert_hip_n_vocab", "bert_hip_ftype", "bert_hip_device", "bert_hip_pooling", "bert_hip_normalize"):
        getattr(L, fn).restype = i32; getattr(L, fn).argtypes = [vp]
    L.bert_vocab_id_to_token.restype = C.c_char_p; L.bert_vocab_id_to_token.argtypes = [vp, i32]
    L.bert_tokenize.restype = None; L.bert_tokenize.argtypes = [vp, C.c_char_p, i32p, i32p, i32]
    L.bert_eval.restype = None; L.bert_eval.argtypes = [vp, i32, i32p, i32, f32p]
    L.bert_eval_batch.restype = None
    L.bert_eval_batch.argtypes = [vp, i32, i32, C.POINTER(i32p), i32p, C.POINTER(f32p)]
    L.bert_encode.restype = None; L.bert_encode.argtypes = [vp, i32, C.c_char_p, f32p]
    L.bert_encode_batch.restype = None
    L.bert_encode_batch.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_char_p), C.POINTER(f32p)]
    L.bert_hip_eval_packed.restype = i32; L.bert_hip_eval_packed.argtypes = [vp, i32p, i32p, i32, f32p]
    L.bert_hip_eval_packed_device.restype = i32
    L.bert_hip_eval_packed_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.bert_hip_eval_hidden.restype = i32; L.bert_hip_eval_hidden.argtypes = [vp, i32p, i32, f32p, f32p]
    L.bert_hip_profile_enable.restype = None; L.bert_hip_profile_enable.argtypes = [vp, i32]
    L.bert_hip_profile_report.restype = i32; L.bert_hip_profile_report.argtypes = [vp, C.c_char_p, i32]
    L.bert_hip_set_option.restype = None; L.bert_hip_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.bert_hip_n_devices.restype = i32; L.bert_hip_n_devices.argtypes = [vp]
    L.bert_hip_encode_batch.restype = i32
    L.bert_hip_encode_batch.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), C.POINTER(f32p)]
    L.bert_hip_eval_packed_gather.restype = i32
    L.bert_hip_eval_packed_gather.argtypes = [vp, i32p, i32p, i32, C.POINTER(vp)]
    L.bert_hip_reserve.restype = i32; L.bert_hip_reserve.argtypes = [vp, i32, i32]
    L.bert_hip_check.restype = i32; L.bert_hip_check.argtypes = [vp]
    L.bert_hip_tokenize_batch.restype = i32
    L.bert_hip_tokenize_batch.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32p, i32p]
    L.bert_hip_version.restype = C.c_char_p
    L.bert_hip_index_create.restype = vp; L.bert_hip_index_create.argtypes = [vp, i32, i32]
    L.bert_hip_index_free.restype = None; L.bert_hip_index_free.argtypes = [vp]
    L.bert_hip_index_size.restype = i32; L.bert_hip_index_size.argtypes = [vp]
    L.bert_hip_index_reserve.restype = i32; L.bert_hip_index_reserve.argtypes = [vp, i32, i32, i32]
    L.bert_hip_index_add.restype = i32; L.bert_hip_index_add.argtypes = [vp, i32, f32p]
    L.bert_hip_index_add_device.restype = i32; L.bert_hip_index_add_device.argtypes = [vp, i32, vp, vp]
    L.bert_hip_index_add_texts.restype = i32; L.bert_hip_index_add_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p)]
    L.bert_hip_index_search.restype = i32; L.bert_hip_index_search.argtypes = [vp, i32, f32p, i32, i32p, f32p]
    L.bert_hip_index_search_device.restype = i32; L.bert_hip_index_search_device.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_index_search_texts.restype = i32
    L.bert_hip_index_search_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32p, f32p]
    L.bert_hip_index_remove.restype = i32; L.bert_hip_index_remove.argtypes = [vp, i32, i32p]
    L.bert_hip_index_n_live.restype = i32; L.bert_hip_index_n_live.argtypes = [vp]
    L.bert_hip_index_search_filtered.restype = i32; L.bert_hip_index_search_filtered.argtypes = [vp, i32, f32p, i32, vp, i32, i32p, f32p]
    L.bert_hip_index_search_filtered_device.restype = i32
    L.bert_hip_index_search_filtered_device.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_index_compact.restype = i32; L.bert_hip_index_compact.argtypes = [vp, i32p]
    L.bert_hip_index_save.restype = i32; L.bert_hip_index_save.argtypes = [vp, C.c_char_p]
    L.bert_hip_index_load.restype = vp; L.bert_hip_index_load.argtypes = [vp, C.c_char_p]
    L.bert_hip_index_rescore.restype = i32; L.bert_hip_index_rescore.argtypes = [vp, i32, f32p, i32, i32p, i32, i32p, f32p]
    L.bert_hip_index_rescore_device.restype = i32; L.bert_hip_index_rescore_device.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_index_search_rescored.restype = i32; L.bert_hip_index_search_rescored.argtypes = [vp, vp, i32, f32p, i32, i32, i32p, f32p]
    L.bert_hip_index_search_rescored_device.restype = i32
    L.bert_hip_index_search_rescored_device.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp]
    L.bert_hip_index_get_rows.restype = i32; L.bert_hip_index_get_rows.argtypes = [vp, i32, i32p, f32p]
    L.bert_hip_index_partition.restype = i32; L.bert_hip_index_partition.argtypes = [vp, i32, f32p]
    L.bert_hip_index_n_lists.restype = i32; L.bert_hip_index_n_lists.argtypes = [vp]
    L.bert_hip_index_partition_centroids.restype = i32; L.bert_hip_index_partition_centroids.argtypes = [vp, f32p]
    L.bert_hip_index_partition_lists.restype = i32; L.bert_hip_index_partition_lists.argtypes = [vp, i32p]
    L.bert_hip_index_kmeans.restype = i32; L.bert_hip_index_kmeans.argtypes = [vp, i32, i32, f32p]
    L.bert_hip_index_search_probed.restype = i32; L.bert_hip_index_search_probed.argtypes = [vp, i32, f32p, i32, i32, i32p, f32p]
    L.bert_hip_index_search_probed_device.restype = i32; L.bert_hip_index_search_probed_device.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp]
    L.bert_hip_index_search_probed_filtered.restype = i32
    L.bert_hip_index_search_probed_filtered.argtypes = [vp, i32, f32p, i32, i32, vp, i32, i32p, f32p]
    L.bert_hip_index_search_probed_filtered_device.restype = i32
    L.bert_hip_index_search_probed_filtered_device.argtypes = [vp, i32, vp, i32, i32, vp, i32, vp, vp, vp]
    L.bert_hip_index_search_rescored_probed.restype = i32
    L.bert_hip_index_search_rescored_probed.argtypes = [vp, vp, i32, f32p, i32, i32, i32, vp, i32, i32p, f32p]
    L.bert_hip_index_search_rescored_probed_device.restype = i32
    L.bert_hip_index_search_rescored_probed_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, i32, vp, vp, vp]
    L.bert_hip_index_partition_save.restype = i32; L.bert_hip_index_partition_save.argtypes = [vp, C.c_char_p]
    L.bert_hip_index_partition_load.restype = i32; L.bert_hip_index_partition_load.argtypes = [vp, C.c_char_p]
    L.bert_hip_eval_packed_grouped.restype = i32; L.bert_hip_eval_packed_grouped.argtypes = [vp, i32p, i32p, i32, i32p, i32, f32p]
    L.bert_hip_eval_packed_grouped_device.restype = i32
    L.bert_hip_eval_packed_grouped_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, i32, vp, vp]
    L.bert_hip_tokenize_long.restype = i32; L.bert_hip_tokenize_long.argtypes = [vp, C.c_char_p, i32p, i32]
    L.bert_hip_plan_windows.restype = i32; L.bert_hip_plan_windows.argtypes = [i32, i32, i32, i32p, i32]
    L.bert_hip_encode_long_batch.restype = i32
    L.bert_hip_encode_long_batch.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32, C.POINTER(f32p), i32p]
    L.bert_hip_index_add_long_texts.restype = i32; L.bert_hip_index_add_long_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32]
    L.bert_hip_eval_packed_tokens_device.restype = i32
    L.bert_hip_eval_packed_tokens_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.bert_hip_eval_packed_tokens.restype = i32; L.bert_hip_eval_packed_tokens.argtypes = [vp, i32p, i32p, i32, i32, f32p, f32p]
    L.bert_hip_encode_tokens_batch.restype = C.c_int64
    L.bert_hip_encode_tokens_batch.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32p, f32p, C.c_int64]
    L.bert_hip_maxsim_device.restype = i32; L.bert_hip_maxsim_device.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, vp, i32, i32, vp, vp]
    L.bert_hip_maxsim.restype = i32; L.bert_hip_maxsim.argtypes = [vp, f32p, i32p, i32, f32p, i32p, i32, i32, i32p, i32, i32, f32p]
    L.bert_hip_n_labels.restype = i32; L.bert_hip_n_labels.argtypes = [vp]
    L.bert_hip_relative_attention.restype = i32; L.bert_hip_relative_attention.argtypes = [vp]
    L.bert_hip_tokenize_pair.restype = i32; L.bert_hip_tokenize_pair.argtypes = [vp, C.c_char_p, C.c_char_p, i32p, i32p, i32p, i32]
    L.bert_hip_eval_packed_typed.restype = i32; L.bert_hip_eval_packed_typed.argtypes = [vp, i32p, i32p, i32p, i32, f32p]
    L.bert_hip_eval_packed_typed_device.restype = i32; L.bert_hip_eval_packed_typed_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.bert_hip_score_packed.restype = i32; L.bert_hip_score_packed.argtypes = [vp, i32p, i32p, i32p, i32, i32, f32p]
    L.bert_hip_score_packed_device.restype = i32; L.bert_hip_score_packed_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.bert_hip_score_pairs.restype = i32
    L.bert_hip_score_pairs.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32, f32p]
    L.bert_hip_has_mlm_head.restype = i32; L.bert_hip_has_mlm_head.argtypes = [vp]
    L.bert_hip_sparse_packed.restype = i32; L.bert_hip_sparse_packed.argtypes = [vp, i32p, i32p, i32, f32p]
    L.bert_hip_sparse_packed_device.restype = i32; L.bert_hip_sparse_packed_device.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.bert_hip_sparse_topk_packed.restype = i32; L.bert_hip_sparse_topk_packed.argtypes = [vp, i32p, i32p, i32, i32, i32p, f32p]
    L.bert_hip_sparse_topk_packed_device.restype = i32; L.bert_hip_sparse_topk_packed_device.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.bert_hip_encode_sparse_batch.restype = i32
    L.bert_hip_encode_sparse_batch.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32p, f32p]
    L.bert_hip_sparse_index_create.restype = vp; L.bert_hip_sparse_index_create.argtypes = [vp, i32, i32, i32]
    L.bert_hip_sparse_index_free.restype = None; L.bert_hip_sparse_index_free.argtypes = [vp]
    L.bert_hip_sparse_index_size.restype = i32; L.bert_hip_sparse_index_size.argtypes = [vp]
    L.bert_hip_sparse_index_reserve.restype = i32; L.bert_hip_sparse_index_reserve.argtypes = [vp, i32, i32, i32]
    L.bert_hip_sparse_index_add.restype = i32; L.bert_hip_sparse_index_add.argtypes = [vp, i32, i32, vp, vp]
    L.bert_hip_sparse_index_add_device.restype = i32; L.bert_hip_sparse_index_add_device.argtypes = [vp, i32, i32, vp, vp, vp]
    L.bert_hip_sparse_index_add_texts.restype = i32; L.bert_hip_sparse_index_add_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p)]
    L.bert_hip_sparse_index_search.restype = i32; L.bert_hip_sparse_index_search.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp]
    L.bert_hip_sparse_index_search_device.restype = i32; L.bert_hip_sparse_index_search_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp]
    L.bert_hip_sparse_index_search_texts.restype = i32
    L.bert_hip_sparse_index_search_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32, vp, vp]
    L.bert_hip_sparse_index_get_rows.restype = i32; L.bert_hip_sparse_index_get_rows.argtypes = [vp, i32, vp, vp, vp]
    L.bert_hip_sparse_index_remove.restype = i32; L.bert_hip_sparse_index_remove.argtypes = [vp, i32, vp]
    L.bert_hip_sparse_index_n_live.restype = i32; L.bert_hip_sparse_index_n_live.argtypes = [vp]
    L.bert_hip_sparse_index_search_filtered.restype = i32
    L.bert_hip_sparse_index_search_filtered.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    L.bert_hip_sparse_index_search_filtered_device.restype = i32
    L.bert_hip_sparse_index_search_filtered_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_sparse_index_rescore.restype = i32; L.bert_hip_sparse_index_rescore.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    L.bert_hip_sparse_index_rescore_device.restype = i32
    L.bert_hip_sparse_index_rescore_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_sparse_index_compact.restype = i32; L.bert_hip_sparse_index_compact.argtypes = [vp, vp]
    L.bert_hip_sparse_index_save.restype = i32; L.bert_hip_sparse_index_save.argtypes = [vp, C.c_char_p]
    L.bert_hip_sparse_index_load.restype = vp; L.bert_hip_sparse_index_load.argtypes = [vp, C.c_char_p]
    L.bert_hip_sparse_index_invert.restype = i32; L.bert_hip_sparse_index_invert.argtypes = [vp]
    L.bert_hip_sparse_index_inverted_rows.restype = i32; L.bert_hip_sparse_index_inverted_rows.argtypes = [vp]
    L.bert_hip_sparse_index_search_inverted.restype = i32
    L.bert_hip_sparse_index_search_inverted.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    L.bert_hip_sparse_index_search_inverted_device.restype = i32
    L.bert_hip_sparse_index_search_inverted_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_sparse_index_search_inverted_texts.restype = i32
    L.bert_hip_sparse_index_search_inverted_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, i32, vp, vp]
    f32 = C.c_float
    L.bert_hip_hybrid_reserve.restype = i32; L.bert_hip_hybrid_reserve.argtypes = [vp, vp, i32, i32, i32]
    L.bert_hip_hybrid_search.restype = i32; L.bert_hip_hybrid_search.argtypes = [vp, vp, i32, vp, i32, vp, vp, f32, f32, vp, i32, i32, vp, vp]
    L.bert_hip_hybrid_search_device.restype = i32
    L.bert_hip_hybrid_search_device.argtypes = [vp, vp, i32, vp, i32, vp, vp, f32, f32, vp, i32, i32, vp, vp, vp]
    L.bert_hip_hybrid_search_texts.restype = i32
    L.bert_hip_hybrid_search_texts.argtypes = [vp, vp, i32, i32, C.POINTER(C.c_char_p), i32, f32, f32, i32, vp, vp]
    # (the same searches over the sparse index's postings: the argument lists of the three above)
    L.bert_hip_dense_sparse_search_inverted.restype = i32
    L.bert_hip_dense_sparse_search_inverted.argtypes = list(L.bert_hip_hybrid_search.argtypes)
    L.bert_hip_dense_sparse_search_inverted_device.restype = i32
    L.bert_hip_dense_sparse_search_inverted_device.argtypes = list(L.bert_hip_hybrid_search_device.argtypes)
    L.bert_hip_dense_sparse_search_inverted_texts.restype = i32
    L.bert_hip_dense_sparse_search_inverted_texts.argtypes = list(L.bert_hip_hybrid_search_texts.argtypes)
    i64 = C.c_int64
    L.bert_hip_token_index_create.restype = vp; L.bert_hip_token_index_create.argtypes = [vp, i32]
    L.bert_hip_token_index_free.restype = None; L.bert_hip_token_index_free.argtypes = [vp]
    L.bert_hip_token_index_size.restype = i32; L.bert_hip_token_index_size.argtypes = [vp]
    L.bert_hip_token_index_n_tokens.restype = i64; L.bert_hip_token_index_n_tokens.argtypes = [vp]
    L.bert_hip_token_index_max_query_tokens.restype = i32; L.bert_hip_token_index_max_query_tokens.argtypes = [vp]
    L.bert_hip_token_index_reserve.restype = i32; L.bert_hip_token_index_reserve.argtypes = [vp, i32, i64, i32, i32, i32]
    L.bert_hip_token_index_add.restype = i32; L.bert_hip_token_index_add.argtypes = [vp, i32, vp, vp]
    L.bert_hip_token_index_add_device.restype = i32; L.bert_hip_token_index_add_device.argtypes = [vp, i32, vp, vp, vp]
    L.bert_hip_token_index_add_texts.restype = i32; L.bert_hip_token_index_add_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p)]
    L.bert_hip_token_index_get_doc.restype = i32; L.bert_hip_token_index_get_doc.argtypes = [vp, i32, vp, i32]
    L.bert_hip_token_index_search.restype = i32; L.bert_hip_token_index_search.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    L.bert_hip_token_index_search_device.restype = i32; L.bert_hip_token_index_search_device.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp]
    L.bert_hip_token_index_search_texts.restype = i32
    L.bert_hip_token_index_search_texts.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32, vp, vp]
    L.bert_hip_token_index_rescore.restype = i32; L.bert_hip_token_index_rescore.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp]
    L.bert_hip_token_index_rescore_device.restype = i32
    L.bert_hip_token_index_rescore_device.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp]
    L.bert_hip_late_index_remove.restype = i32; L.bert_hip_late_index_remove.argtypes = [vp, i32, vp]
    L.bert_hip_late_index_n_live.restype = i32; L.bert_hip_late_index_n_live.argtypes = [vp]
    L.bert_hip_late_index_n_live_tokens.restype = i64; L.bert_hip_late_index_n_live_tokens.argtypes = [vp]
    L.bert_hip_late_index_search_filtered.restype = i32; L.bert_hip_late_index_search_filtered.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp]
    L.bert_hip_late_index_search_filtered_device.restype = i32
    L.bert_hip_late_index_search_filtered_device.argtypes = [vp, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp]
    L.bert_hip_late_index_compact.restype = i32; L.bert_hip_late_index_compact.argtypes = [vp, vp]
    L.bert_hip_late_index_save.restype = i32; L.bert_hip_late_index_save.argtypes = [vp, C.c_char_p]
    L.bert_hip_late_index_load.restype = vp; L.bert_hip_late_index_load.argtypes = [vp, C.c_char_p]
    L.bert_hip_late_index_create.restype = vp; L.bert_hip_late_index_create.argtypes = [vp, i32, i32]
    L.bert_hip_late_index_dtype.restype = i32; L.bert_hip_late_index_dtype.argtypes = [vp]
    L.bert_hip_late_index_get_codes.restype = i32; L.bert_hip_late_index_get_codes.argtypes = [vp, i32, vp, vp, i32]


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build the HIP extension first "
                           f"(python -c 'import __graft_entry__ as g; g.build()' or make -C bert.cpp_amd)")
    L = C.CDLL(LIB_PATH)
    _declare_product_abi(L)
    _lib = L
    return L


_test_lib = None


def test_lib() -> C.CDLL:
    """libbert_test.so: the product's objects plus the op-level test hooks of include/bert_hip_test.h."""
    global _test_lib
    if _test_lib is not None:
        return _test_lib
    if not os.path.exists(TEST_LIB_PATH):
        raise RuntimeError(f"{TEST_LIB_PATH} not found: build it first (make -C bert.cpp_amd)")
    L = C.CDLL(TEST_LIB_PATH)
    _declare_product_abi(L)
    vp, i32, i32p = C.c_void_p, C.c_int32, C.POINTER(C.c_int32)
    L.bert_hip_test_gemm.restype = i32
    L.bert_hip_test_gemm.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, vp]
    L.bert_hip_test_gemm_lnfold.restype = i32
    L.bert_hip_test_gemm_lnfold.argtypes = [i32, i32, i32, i32] + [vp] * 10 + [i32, vp, vp, vp]
    L.bert_hip_test_attention.restype = i32
    L.bert_hip_test_attention.argtypes = [i32, i32p, i32, i32, vp, i32, vp]
    L.bert_hip_test_attention_bias.restype = i32
    L.bert_hip_test_attention_bias.argtypes = [i32, i32p, i32, i32, vp, i32, vp, vp, i32, vp]
    L.bert_hip_test_rel_bias_table.restype = i32
    L.bert_hip_test_rel_bias_table.argtypes = [vp, i32, i32, vp]
    L.bert_hip_test_qkv_attention.restype = i32
    L.bert_hip_test_qkv_attention.argtypes = [i32, i32p, i32, i32, vp, vp, i32, vp, i32, vp]
    L.bert_hip_test_layer_tail.restype = i32
    L.bert_hip_test_layer_tail.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.bert_hip_test_skinny_tail.restype = i32
    L.bert_hip_test_skinny_tail.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.bert_hip_test_skinny_qkv.restype = i32
    L.bert_hip_test_skinny_qkv.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, vp, C.c_uint32, vp, vp]
    L.bert_hip_test_embed_ln.restype = i32
    L.bert_hip_test_embed_ln.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, i32p, i32p, i32, i32, vp]
    L.bert_hip_test_embed_ln_lanes.restype = i32
    L.bert_hip_test_embed_ln_lanes.argtypes = L.bert_hip_test_embed_ln.argtypes
    L.bert_hip_test_layernorm.restype = i32
    L.bert_hip_test_layernorm.argtypes = [i32, i32, vp, vp, vp, vp]
    L.bert_hip_test_pool_normalize.restype = i32
    L.bert_hip_test_pool_normalize.argtypes = [i32, vp, i32p, i32, i32, vp, i32p]
    L.bert_hip_test_pool.restype = i32
    L.bert_hip_test_pool.argtypes = [i32, vp, i32p, i32, i32, i32, i32, vp, i32p]
    L.bert_hip_test_f32_gemm.restype = i32
    L.bert_hip_test_f32_gemm.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, vp]
    L.bert_hip_test_f32_attention.restype = i32
    L.bert_hip_test_f32_attention.argtypes = [i32, i32p, i32, i32, i32, vp, vp]
    L.bert_hip_test_f32_attention_bias.restype = i32
    L.bert_hip_test_f32_attention_bias.argtypes = [i32, i32p, i32, i32, i32, vp, vp, vp, i32]
    L.bert_hip_test_f32_layernorm.restype = i32
    L.bert_hip_test_f32_layernorm.argtypes = [i32, i32, vp, vp, vp, vp]
    L.bert_hip_test_f32_embed_ln.restype = i32
    L.bert_hip_test_f32_embed_ln.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32p, i32p, i32, i32, vp]
    L.bert_hip_test_f32_pool.restype = i32
    L.bert_hip_test_f32_pool.argtypes = [i32, vp, i32p, i32, i32, i32, i32, vp, i32p]
    L.bert_hip_test_model_digest.restype = i32
    L.bert_hip_test_model_digest.argtypes = [C.c_char_p, i32p, C.POINTER(C.c_uint64)]
    L.bert_hip_test_pack_weight.restype = i32
    L.bert_hip_test_pack_weight.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, C.c_int64]
    L.bert_hip_test_shard_bounds.restype = None
    L.bert_hip_test_shard_bounds.argtypes = [i32p, i32, i32, i32p]
    L.bert_hip_test_build_windows.restype = i32
    L.bert_hip_test_build_windows.argtypes = [i32p, i32, i32p]
    L.bert_hip_test_max_windows.restype = i32
    L.bert_hip_test_max_windows.argtypes = [i32, i32]
    L.bert_hip_test_set_window_slots.restype = i32
    L.bert_hip_test_set_window_slots.argtypes = [i32]
    L.bert_hip_test_set_pad.restype = None
    L.bert_hip_test_set_pad.argtypes = [C.c_uint32, C.c_uint32]
    L.bert_hip_test_build_windows_device.restype = i32
    L.bert_hip_test_build_windows_device.argtypes = [i32p, i32, i32p]
    L.bert_hip_test_shard_threads_created.restype = C.c_int64
    L.bert_hip_test_shard_threads_created.argtypes = []
    L.bert_hip_test_dispatch.restype = i32
    L.bert_hip_test_dispatch.argtypes = [i32p, i32p, i32, i32, i32, C.POINTER(C.c_float)]
    L.bert_hip_test_parse_devices.restype = i32
    L.bert_hip_test_parse_devices.argtypes = [C.c_char_p, i32, i32, i32p, C.c_char_p, i32]
    L.bert_hip_test_gather_runs.restype = i32
    L.bert_hip_test_gather_runs.argtypes = [i32p, i32, C.c_int64, i32p]
    L.bert_hip_test_encode_groups.restype = i32
    L.bert_hip_test_encode_groups.argtypes = [i32, i32p, i32]
    L.bert_hip_test_tokenize_pack.restype = i32
    L.bert_hip_test_tokenize_pack.argtypes = [vp, i32, i32, C.POINTER(C.c_char_p), i32p, i32p, i32p, i32p, i32]
    L.bert_hip_test_index_header.restype = i32
    L.bert_hip_test_index_header.argtypes = [C.c_char_p, i32, C.c_int64, C.POINTER(C.c_uint32), C.c_char_p, i32]
    L.bert_hip_test_partition_header.restype = i32
    L.bert_hip_test_partition_header.argtypes = [C.c_char_p, i32, C.c_int64, C.POINTER(C.c_uint32), C.c_char_p, i32]
    L.bert_hip_test_sparse_postings_geometry.restype = i32
    L.bert_hip_test_sparse_postings_geometry.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.bert_hip_test_sparse_postings_segment.restype = i32
    L.bert_hip_test_sparse_postings_segment.argtypes = [vp, i32, i32, vp, vp, vp, C.POINTER(i32)]
    L.bert_hip_test_sparse_index_header.restype = i32
    L.bert_hip_test_sparse_index_header.argtypes = [C.c_char_p, i32, C.c_int64, C.POINTER(C.c_uint32), C.c_char_p, i32]
    L.bert_hip_test_sparse_index_body.restype = i32
    L.bert_hip_test_sparse_index_body.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_int64, C.c_char_p, i32]
    L.bert_hip_test_build_lists.restype = i32
    L.bert_hip_test_build_lists.argtypes = [i32p, i32, i32, i32p, i32p]
    L.bert_hip_test_group_pool.restype = i32
    L.bert_hip_test_group_pool.argtypes = [vp, i32, i32p, i32p, i32, i32, i32, vp, i32p]
    L.bert_hip_test_token_rows.restype = i32
    L.bert_hip_test_token_rows.argtypes = [vp, i32, i32, i32, i32p, i32, i32, i32, vp]
    L.bert_hip_test_embed_ln_typed.restype = i32
    L.bert_hip_test_embed_ln_typed.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, i32p, i32p, i32, i32, vp, i32, vp]
    L.bert_hip_test_cls_head.restype = i32
    L.bert_hip_test_cls_head.argtypes = [i32, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, vp]
    L.bert_hip_test_sparse_vocab.restype = i32
    L.bert_hip_test_sparse_vocab.argtypes = [i32, i32, i32, vp, i32, vp, i32, vp, i32p, i32, i32, i32, vp]
    L.bert_hip_test_sparse_topk.restype = i32
    L.bert_hip_test_sparse_topk.argtypes = [vp, i32, i32, i32, vp, vp]
    L.bert_hip_test_sparse_vocab_geometry.restype = i32
    L.bert_hip_test_sparse_vocab_geometry.argtypes = [i32, i32, i32, i32, i32, i32p]
    L.bert_hip_test_attention_grid.restype = i32
    L.bert_hip_test_attention_grid.argtypes = [i32, i32, i32, i32, i32p, i32p]
    L.bert_hip_test_sparse_scan_geometry.restype = i32
    L.bert_hip_test_sparse_scan_geometry.argtypes = [i32, i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.bert_hip_test_sparse_scan_geometry_qb.restype = i32
    L.bert_hip_test_sparse_scan_geometry_qb.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int64)]
    L.bert_hip_test_index_plan.restype = i32
    L.bert_hip_test_index_plan.argtypes = [i32, i32, i32, i32p]
    L.bert_hip_test_hybrid_chunk.restype = i32
    L.bert_hip_test_hybrid_chunk.argtypes = [i32, i32, i32, C.POINTER(C.c_int64)]
    L.bert_hip_test_token_index_plan.restype = i32
    L.bert_hip_test_token_index_plan.argtypes = [i32, i32, i32, i32p]
    L.bert_hip_test_late_index_header.restype = i32
    L.bert_hip_test_late_index_header.argtypes = [C.c_char_p, i32, C.c_int64, C.POINTER(C.c_uint32), C.c_char_p, i32]
    L.bert_hip_test_late_index_body.restype = i32
    L.bert_hip_test_late_index_body.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_int64, C.c_char_p, i32]
    _test_lib = L
    return L


def test_embed_ln(table_type: int, word_bytes, type_bytes, pos_bytes, H: int, gamma, beta, tokens, cu_seqlens, max_len: int = 0, lanes: bool = False) -> np.ndarray:
    """Tables as file-layout bytes (the position table has as many rows as pos_bytes holds); max_len: the promise the launch is made
    under, 0 = the longest sentence.  Returns float16 [T, H]."""
    wb, tb, pb = (np.ascontiguousarray(a) for a in (word_bytes, type_bytes, pos_bytes))
    rb = {0: 4 * H, 1: 2 * H, 2: H // 32 * 18, 3: H // 32 * 20}[table_type]
    g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
    toks = np.ascontiguousarray(tokens, dtype=np.int32); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    assert len(toks) == int(cu[-1]) and tb.nbytes == 2 * rb and g.shape == (H,) and b.shape == (H,)
    out = np.zeros((len(toks), H), dtype=np.float16)
    entry = getattr(test_lib(), "bert_hip_test_embed_ln_lanes" if lanes else "bert_hip_test_embed_ln")
    r = entry(table_type, H, wb.nbytes // rb, pb.nbytes // rb, wb.ctypes.data, tb.ctypes.data, pb.ctypes.data,
              g.ctypes.data, b.ctypes.data, _i32p(toks), _i32p(cu), len(cu) - 1, max_len, out.ctypes.data)
    if lanes and r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_embed_ln{'_lanes' if lanes else ''} failed: {r}")
    return out


def test_embed_ln_lanes(table_type: int, word_bytes, type_bytes, pos_bytes, H: int, gamma, beta, tokens, cu_seqlens, max_len: int = 0):
    """The lane-order form (launch_embed_ln_lanes) on test_embed_ln's arguments: the float16 [T, H] halves as the kernel stored them
    (tests/lane_order.py puts them back into rows), or None where the launcher declines the shape and launches nothing."""
    return test_embed_ln(table_type, word_bytes, type_bytes, pos_bytes, H, gamma, beta, tokens, cu_seqlens, max_len, lanes=True)


EMBED_FORMS = {"grid": 0, "search": 1, "generic": 2, "lanes": 3, "f32": 4}


def test_embed_ln_typed(table_type: int, word_bytes, type_bytes, pos_bytes, H: int, gamma, beta, tokens, cu_seqlens, first_len, form: str,
                        max_len: int = 0):
    """An embedding kernel with token types (bert_hip_test.h): test_embed_ln's arguments, first_len (int per sentence, or None: the
    untyped instantiation) and the form, a key of EMBED_FORMS.  float16 [T, H] (float32 for "f32"; "lanes": as the kernel stored them), or
    None where the form does not take the shape."""
    wb, tb, pb = (np.ascontiguousarray(a) for a in (word_bytes, type_bytes, pos_bytes))
    rb = {0: 4 * H, 1: 2 * H, 2: H // 32 * 18, 3: H // 32 * 20}[table_type]
    g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
    toks = np.ascontiguousarray(tokens, dtype=np.int32); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    fl = None if first_len is None else np.ascontiguousarray(first_len, dtype=np.int32)
    assert len(toks) == int(cu[-1]) and tb.nbytes == 2 * rb and g.shape == (H,) and b.shape == (H,) and (fl is None or len(fl) == len(cu) - 1)
    out = np.zeros((len(toks), H), dtype=np.float32 if form == "f32" else np.float16)
    r = test_lib().bert_hip_test_embed_ln_typed(table_type, H, wb.nbytes // rb, pb.nbytes // rb, wb.ctypes.data, tb.ctypes.data, pb.ctypes.data,
                                                g.ctypes.data, b.ctypes.data, _i32p(toks), _i32p(cu), len(cu) - 1, max_len,
                                                None if fl is None else fl.ctypes.data, EMBED_FORMS[form], out.ctypes.data)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_embed_ln_typed failed: {r}")
    return out


def test_cls_head(rows, Wp, bp, Wc, bc, flags: int = 0, form: str = "mfma"):
    """The classification head on its own: rows float32 [B, H]; Wp [H, H] float16 or float32 (its dtype says which image the kernel
    reads); bp [H], Wc [n_labels, H], bc [n_labels] float32; form "mfma" or "plain".  float32 [B, n_labels], or None where the form does
    not take the shape."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    Wp = np.ascontiguousarray(Wp)
    assert Wp.dtype in (np.float16, np.float32)
    bp, Wc, bc = (np.ascontiguousarray(a, dtype=np.float32) for a in (bp, Wc, bc))
    B, H = rows.shape
    NL = Wc.shape[0]
    assert Wp.shape == (H, H) and bp.shape == (H,) and Wc.shape == (NL, H) and bc.shape == (NL,)
    out = np.full((B, NL), np.nan, dtype=np.float32)
    r = test_lib().bert_hip_test_cls_head(B, H, NL, rows.ctypes.data, Wp.ctypes.data, int(Wp.dtype == np.float32), bp.ctypes.data, Wc.ctypes.data,
                                          bc.ctypes.data, flags, {"mfma": 0, "plain": 1}[form], out.ctypes.data)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_cls_head failed: {r}")
    return out


def test_sparse_vocab(t, e, bias, cu_seqlens, form: str = "mfma", s0: int = 0, ns: Optional[int] = None):
    """The vocabulary launch of the learned sparse embeddings on its own (bert_hip_test.h): t [T, H] token rows and e [V, H] vocabulary
    rows, float16 or float32 (the dtype says which operand the kernel reads), bias [V]; sentences s0 .. s0 + ns - 1 of cu_seqlens.
    float32 [ns, V], or None where the form does not take the shape."""
    t, e = np.ascontiguousarray(t), np.ascontiguousarray(e)
    assert t.dtype in (np.float16, np.float32) and e.dtype in (np.float16, np.float32)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    (T, H), V, B = t.shape, e.shape[0], len(cu) - 1
    ns = B - s0 if ns is None else ns
    assert e.shape == (V, H) and bias.shape == (V,) and int(cu[-1]) == T
    out = np.full((ns, V), np.nan, dtype=np.float32)
    r = test_lib().bert_hip_test_sparse_vocab({"mfma": 0, "plain": 1}[form], H, V, t.ctypes.data, int(t.dtype == np.float32), e.ctypes.data,
                                              int(e.dtype == np.float32), bias.ctypes.data, _i32p(cu), B, s0, ns, out.ctypes.data)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_sparse_vocab failed: {r}")
    return out


def test_sparse_vocab_geometry(H: int, V: int, T: int, ns: int, max_len: int):
    """The grid of the matrix-core vocabulary launch (bert_hip_test.h; no GPU): {"tile", "n_tiles", "slab_blocks", "n_slabs"} for T packed
    tokens of which ns sentences of at most max_len tokens are served, or None where the launcher refuses the shape."""
    g = (C.c_int32 * 4)()
    r = test_lib().bert_hip_test_sparse_vocab_geometry(H, V, T, ns, max_len, g)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_sparse_vocab_geometry failed: {r}")
    return dict(zip(("tile", "n_tiles", "slab_blocks", "n_slabs"), (int(x) for x in g)))


def test_sparse_scan_geometry(dtype: int, n_vocab: int, n_rows: int, nq: int, k: int, qb: Optional[int] = None):
    """How the sparse index's scan cuts a search (bert_hip_test_sparse_scan_geometry; no GPU): a dict of qb, n_qtiles, n_slices, slice_rows,
    L and lds, or None where the plan refuses.  qb: the value of the tuning key "sparse_index_qb" the plan is made under
    (bert_hip_test_sparse_scan_geometry_qb); None = the key unset."""
    g = (C.c_int64 * 6)()
    if qb is None:
        r = test_lib().bert_hip_test_sparse_scan_geometry(dtype, n_vocab, n_rows, nq, k, g)
    else:
        r = test_lib().bert_hip_test_sparse_scan_geometry_qb(dtype, n_vocab, n_rows, nq, k, qb, g)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_sparse_scan_geometry failed: {r}")
    return dict(qb=g[0], n_qtiles=g[1], n_slices=g[2], slice_rows=g[3], L=g[4], lds=g[5])


def test_sparse_postings_geometry(dtype: int, n_vocab: int, n_rows: int, nq: int, k: int, seg: int, qb: int = 0):
    """How the sparse index's inverted search cuts a chunk of queries (bert_hip_test_sparse_postings_geometry; no GPU): a dict of qb,
    n_qtiles, n_slices, slice_segs, L, max_slices and lds, or None where the plan refuses.  seg: rows per segment; qb: the value of the
    tuning key "sparse_index_qb" (0 = unset)."""
    g = (C.c_int64 * 7)()
    r = test_lib().bert_hip_test_sparse_postings_geometry(dtype, n_vocab, n_rows, nq, k, seg, qb, g)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_sparse_postings_geometry failed: {r}")
    return dict(qb=g[0], n_qtiles=g[1], n_slices=g[2], slice_segs=g[3], L=g[4], max_slices=g[5], lds=g[6])


def test_sparse_postings_segment(index: "BertSparseIndex", segment: int):
    """One segment of an index's postings (bert_hip_test_sparse_postings_segment; the index of a BertModel(test_routes=True)):
    (off [n_vocab + 1] uint32, rows [total] int32 — row numbers inside the segment —, weights [total] float32, seg_rows)."""
    off = np.zeros(index.n_vocab + 1, dtype=np.uint32)
    cap = 16384 * index.width
    rows = np.zeros(cap, dtype=np.int32)
    w = np.zeros(cap, dtype=np.float32)
    seg_rows = C.c_int32(0)
    r = test_lib().bert_hip_test_sparse_postings_segment(index.ix, segment, cap, off.ctypes.data, rows.ctypes.data, w.ctypes.data, C.byref(seg_rows))
    if r < 0:
        raise RuntimeError(f"bert_hip_test_sparse_postings_segment failed: {r}")
    return off, rows[:r].copy(), w[:r].copy(), int(seg_rows.value)


def test_index_plan(n_rows: int, nq: int, k: int):
    """How the embedding index's search cuts a chunk of nq queries (bert_hip_test_index_plan; no GPU): a dict of nqt, slices, slice_rows and
    L, or None where the hook refuses the arguments."""
    g = (C.c_int32 * 4)()
    r = test_lib().bert_hip_test_index_plan(n_rows, nq, k, g)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_index_plan failed: {r}")
    return dict(nqt=g[0], slices=g[1], slice_rows=g[2], L=g[3])


def test_hybrid_chunk(n_rows: int, nq: int, pref: int = 0):
    """How a hybrid search chunks nq queries over n_rows rows (bert_hip_test_hybrid_chunk; no GPU): (HC, ld), or None where the hook
    refuses.  pref: the value of the tuning key "hybrid_chunk_queries" (0 = unset)."""
    out = (C.c_int64 * 2)()
    r = test_lib().bert_hip_test_hybrid_chunk(n_rows, nq, pref, out)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_hybrid_chunk failed: {r}")
    return int(out[0]), int(out[1])


def test_token_index_plan(n_docs: int, nq: int, pref: int = 0):
    """How a token index's scan cuts nq queries over n_docs documents (bert_hip_test_token_index_plan; no GPU): (n_slices, slice_docs),
    or None where the hook refuses.  pref: the value of the tuning key "token_index_slices" (0 = planned)."""
    out = (C.c_int32 * 2)()
    r = test_lib().bert_hip_test_token_index_plan(n_docs, nq, pref, out)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_token_index_plan failed: {r}")
    return int(out[0]), int(out[1])


def test_attention_grid(n_sentences: int, n_head: int, d_head: int, max_len: int):
    """(threads, grid, items) of test_attention's matrix-core launch on the current device (bert_hip_test.h): 512 threads are the
    persistent form, whose workgroups walk items `grid` apart.  (0, 0, 0) for a shape the launcher refuses."""
    threads, items = C.c_int32(0), C.c_int32(0)
    grid = test_lib().bert_hip_test_attention_grid(n_sentences, n_head, d_head, max_len, C.byref(threads), C.byref(items))
    if grid < 0:
        raise RuntimeError(f"bert_hip_test_attention_grid failed: {grid}")
    return int(threads.value), int(grid), int(items.value)


def test_sparse_topk(w, k: int):
    """The top-k launch on its own: w float32 [n, V] -> (ids int32 [n, k], weights float32 [n, k]), or None where it refuses k or V."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, V = w.shape
    ids = np.full((n, max(k, 1)), -7, dtype=np.int32)
    wt = np.full((n, max(k, 1)), np.nan, dtype=np.float32)
    r = test_lib().bert_hip_test_sparse_topk(w.ctypes.data, n, V, k, ids.ctypes.data, wt.ctypes.data)
    if r == -2:
        return None
    if r != 0:
        raise RuntimeError(f"bert_hip_test_sparse_topk failed: {r}")
    return ids, wt


def test_layernorm(x: np.ndarray, gamma, beta) -> np.ndarray:
    """launch_layernorm on f16 rows x [T, H] (in place on the device, as in the engine); returns float16 [T, H]."""
    x = np.ascontiguousarray(x, dtype=np.float16)
    g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
    assert g.shape == (x.shape[1],) and b.shape == (x.shape[1],)
    out = np.zeros_like(x)
    r = test_lib().bert_hip_test_layernorm(x.shape[0], x.shape[1], x.ctypes.data, g.ctypes.data, b.ctypes.data, out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_layernorm failed: {r}")
    return out


def test_pool_normalize(x: np.ndarray, cu_seqlens, max_len: int):
    x = np.ascontiguousarray(x, dtype=np.float16); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros((len(cu) - 1, x.shape[1]), dtype=np.float32)
    st = np.zeros(1, dtype=np.int32)
    r = test_lib().bert_hip_test_pool_normalize(x.shape[1], x.ctypes.data, _i32p(cu), len(cu) - 1, max_len, out.ctypes.data, _i32p(st))
    if r != 0:
        raise RuntimeError(f"bert_hip_test_pool_normalize failed: {r}")
    return out, int(st[0])


def test_pool(x: np.ndarray, cu_seqlens, max_len: int, pooling: str = "mean", normalize: bool = True):
    """The pooling kernel under a context's settings: pooling "mean" | "cls"; returns (rows [n_sentences, H] f32, status word)."""
    x = np.ascontiguousarray(x, dtype=np.float16); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros((len(cu) - 1, x.shape[1]), dtype=np.float32)
    st = np.zeros(1, dtype=np.int32)
    r = test_lib().bert_hip_test_pool(x.shape[1], x.ctypes.data, _i32p(cu), len(cu) - 1, max_len, {"mean": 0, "cls": 1}[pooling],
                                      int(bool(normalize)), out.ctypes.data, _i32p(st))
    if r != 0:
        raise RuntimeError(f"bert_hip_test_pool failed: {r}")
    return out, int(st[0])


def test_group_pool(rows: np.ndarray, weights, group_cu, raw: bool, out: Optional[np.ndarray] = None):
    """launch_group_pool on chosen rows [n_rows, H] f32 and weights [n_rows] (None: 1 each); group g = rows group_cu[g] .. group_cu[g + 1]
    - 1 (the rows around the groups are the caller's to poison).  out: the buffer as the kernel finds it, [n_groups, H] f32 (None:
    NaNs).  Returns (rows [n_groups, H] f32, status word)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32); g = np.ascontiguousarray(group_cu, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
    assert rows.ndim == 2 and (w is None or w.shape == (rows.shape[0],))
    if out is None:
        out = np.full((len(g) - 1, rows.shape[1]), np.nan, dtype=np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (len(g) - 1, rows.shape[1])
    st = np.zeros(1, dtype=np.int32)
    r = test_lib().bert_hip_test_group_pool(rows.ctypes.data, rows.shape[0], None if w is None else _i32p(w), _i32p(g), len(g) - 1, rows.shape[1],
                                            int(bool(raw)), out.ctypes.data, _i32p(st))
    if r != 0:
        raise RuntimeError(f"bert_hip_test_group_pool failed: {r}")
    return out, int(st[0])


def test_token_rows(x: np.ndarray, cu_seqlens, max_len: int, normalize: bool = True, f16_out: bool = False) -> np.ndarray:
    """launch_token_rows on final states x [T, H], float16 or float32 (the f32 route's); returns the rows [T, H], float32 or (f16_out)
    float16.  Under test_pad the device copy's rows behind T and the output beforehand hold the patterns."""
    assert x.dtype in (np.float16, np.float32) and x.ndim == 2
    x = np.ascontiguousarray(x); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros(x.shape, dtype=np.float16 if f16_out else np.float32)
    r = test_lib().bert_hip_test_token_rows(x.ctypes.data, int(x.dtype == np.float32), x.shape[0], x.shape[1], _i32p(cu), len(cu) - 1, max_len,
                                            int(bool(normalize)) | 2 * int(bool(f16_out)), out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_token_rows failed: {r}")
    return out


def plan_windows(n_tokens: int, window: int, stride: int) -> List[int]:
    """bert_hip_plan_windows: the windows' start offsets among the INNER ids of a text of n_tokens ids (no context, no GPU)."""
    n = lib().bert_hip_plan_windows(n_tokens, window, stride, None, 0)
    if n < 0:
        raise ValueError(f"bert_hip_plan_windows({n_tokens}, {window}, {stride}) = {n}")
    starts = np.zeros(n, dtype=np.int32)
    assert lib().bert_hip_plan_windows(n_tokens, window, stride, _i32p(starts), n) == n
    return starts.tolist()


def model_digest(path: str):
    """(n_tensors, legacy_q4, digest) of a model file as the product's parser sees it (no GPU needed)."""
    leg = C.c_int32(0)
    dig = C.c_uint64(0)
    n = test_lib().bert_hip_test_model_digest(path.encode(), C.byref(leg), C.byref(dig))
    if n < 0:
        raise RuntimeError("model file rejected (see stderr)")
    return n, bool(leg.value), int(dig.value)


PACK_FORMS = {"f16": 0, "f16_kperm": 1, "q4_nibbles": 2, "q4_scales": 3, "ln_fold": 4, "ln_fold_stats": 5, "gamma_beta_bias": 6, "table_f32": 7}


def pack_weight(W, wtype: int, N: int, K: int, form: str, gamma=None, beta=None, bias=None, stack3: bool = False) -> np.ndarray:
    """The bytes of one weight image as the engine's host code packs it (no GPU needed): W is the tensor in its file layout."""
    Wb = np.ascontiguousarray(W)
    f32 = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (gamma, beta, bias)]
    out = np.zeros((N + 127) // 128 * 128 * max(K, 16) * 4, dtype=np.uint8)
    n = test_lib().bert_hip_test_pack_weight(Wb.ctypes.data, wtype, N, K, PACK_FORMS[form] | (0x100 if stack3 else 0),
                                             *(None if a is None else a.ctypes.data for a in f32), out.ctypes.data, out.nbytes)
    if n < 0:
        raise RuntimeError(f"bert_hip_test_pack_weight failed: {n}")
    return out[:n].copy()


def shard_bounds(cu_seqlens: np.ndarray, n_shards: int) -> List[int]:
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros(n_shards + 1, dtype=np.int32)
    test_lib().bert_hip_test_shard_bounds(_i32p(cu), len(cu) - 1, n_shards, _i32p(out))
    return out.tolist()


def build_windows(cu_seqlens: np.ndarray, device: bool = False) -> List[tuple]:
    """{first sentence, count} windows of 128 token slots: the host builder, or (device=True, needs a GPU) the kernel."""
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros(2 * max(len(cu) - 1, 1), dtype=np.int32)
    f = test_lib().bert_hip_test_build_windows_device if device else test_lib().bert_hip_test_build_windows
    n = f(_i32p(cu), len(cu) - 1, _i32p(out))
    if n < 0:
        raise RuntimeError("bert_hip_test_build_windows_device failed")
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def set_window_slots(slots: int) -> int:
    """Place granularity of the windows in libbert_test.so (its own copy of the setting; a context's: set_option "window_slots")."""
    return int(test_lib().bert_hip_test_set_window_slots(slots))


@contextlib.contextmanager
def test_pad(pattern16: int, pattern32: int):
    """While the block runs, the batch-route op entries (test_gemm, test_gemm_lnfold, test_attention, test_qkv_attention,
    test_layer_tail, test_embed_ln, test_layernorm) and the f32 route's (test_f32_*) fill their padding rows and every output / intermediate buffer with these bit patterns before they launch
    (include/bert_hip_test.h bert_hip_test_set_pad); zeros again afterwards."""
    L = test_lib()
    L.bert_hip_test_set_pad(pattern16, pattern32)
    try:
        yield
    finally:
        L.bert_hip_test_set_pad(0, 0)


def max_windows(n_sentences: int, n_tokens: int) -> int:
    return int(test_lib().bert_hip_test_max_windows(n_sentences, n_tokens))


def dispatch_stub(tokens: np.ndarray, cu_seqlens: np.ndarray, n_shards: int, H: int = 4, throw: bool = False) -> np.ndarray:
    tokens = np.ascontiguousarray(tokens, dtype=np.int32)
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.full((len(cu) - 1, abs(H)), np.nan, dtype=np.float32)
    r = test_lib().bert_hip_test_dispatch(_i32p(tokens), _i32p(cu), len(cu) - 1, n_shards, -H if throw else H, _f32p(out))
    if r != 0:
        raise RuntimeError(f"bert_hip_test_dispatch failed: {r}")
    return out


def shard_threads_created() -> int:
    return int(test_lib().bert_hip_test_shard_threads_created())


def parse_devices(spec: Optional[bytes], n_devices: int, current: int = 0):
    """(devices, None) or (None, message): the device list of BERT_HIP_DEVICES as the context's loader reads it (no GPU needed)."""
    devs = np.zeros(max(n_devices, 1), dtype=np.int32)
    err = C.create_string_buffer(512)
    n = test_lib().bert_hip_test_parse_devices(spec, n_devices, current, _i32p(devs), err, len(err))
    return (None, err.value.decode()) if n < 0 else (devs[:n].tolist(), None)


def gather_runs(cu_seqlens: np.ndarray, tokens_per_run: int) -> List[int]:
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros(len(cu), dtype=np.int32)
    n = test_lib().bert_hip_test_gather_runs(_i32p(cu), len(cu) - 1, tokens_per_run, _i32p(out))
    return out[:n].tolist()


def encode_groups(n_inputs: int) -> List[int]:
    out = np.zeros(1024, dtype=np.int32)
    n = test_lib().bert_hip_test_encode_groups(n_inputs, _i32p(out), len(out))
    assert n <= len(out)
    return out[:n].tolist()


def tokenize_pack(model: "BertModel", texts: Sequence[bytes], n_threads: int, counts=None):
    """(n_ok, counts, cu, packed ids) of the text entry points' tokenize + pack step; `model` must live in libbert_test.so
    (test_routes=True).  counts: pack with these counts instead of the tokenizer's."""
    n, N = len(texts), model.n_max_tokens
    arr = (C.c_char_p * n)(*texts)
    cnt = np.zeros(n, dtype=np.int32)
    cu = np.full(n + 1, -1, dtype=np.int32)
    packed = np.full(n * N, -1, dtype=np.int32)
    given = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
    n_ok = test_lib().bert_hip_test_tokenize_pack(model.ctx, n_threads, n, arr, None if given is None else _i32p(given), _i32p(cnt),
                                                  _i32p(cu), _i32p(packed), len(packed))
    if n_ok < 0:
        raise RuntimeError("bert_hip_test_tokenize_pack failed")
    return n_ok, cnt.tolist(), cu[:n_ok + 1].tolist(), packed[:cu[n_ok]].tolist()


def _f32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class BertModel:
    """Mirror of the reference's Python `BertModel` wrapper (examples/sample_dylib.py:12-59)."""

    def __init__(self, fname: str, tokenizer_only: bool = False, test_routes: bool = False):
        # test_routes: the context lives in libbert_test.so, whose engine also understands the whole-model "naive" cross-check route
        self.lib = test_lib() if test_routes else lib()
        load = self.lib.bert_hip_load_tokenizer if tokenizer_only else self.lib.bert_load_from_file
        self.ctx = load(fname.encode("utf-8"))
        if not self.ctx:
            raise RuntimeError(f"bert_load_from_file('{fname}') failed (see stderr)")
        self.n_embd = self.lib.bert_n_embd(self.ctx)
        self.n_max_tokens = self.lib.bert_n_max_tokens(self.ctx)
        self.n_layer = self.lib.bert_hip_n_layer(self.ctx)
        self.n_vocab = self.lib.bert_hip_n_vocab(self.ctx)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.bert_free(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- bert.h ---------------------------------------------------------------------------
    def tokenize(self, text: str | bytes, n_max_tokens: Optional[int] = None) -> List[int]:
        n_max = n_max_tokens or self.n_max_tokens
        buf = (C.c_int32 * max(n_max, 2))()
        n = C.c_int32(0)
        data = text if isinstance(text, bytes) else text.encode("utf-8")
        self.lib.bert_tokenize(self.ctx, data, buf, C.byref(n), n_max)
        return list(buf[: n.value])

    def tokenize_batch(self, texts: Sequence[str | bytes], n_threads: int = 6) -> List[List[int]]:
        n, N = len(texts), self.n_max_tokens
        arr = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        toks = np.zeros((n, N), dtype=np.int32)
        cnt = np.zeros(n, dtype=np.int32)
        if self.lib.bert_hip_tokenize_batch(self.ctx, n_threads, n, arr, _i32p(toks), _i32p(cnt)) != 0:
            raise RuntimeError("bert_hip_tokenize_batch failed")
        return [toks[i, : cnt[i]].tolist() for i in range(n)]

    def id_to_token(self, i: int) -> bytes:
        return self.lib.bert_vocab_id_to_token(self.ctx, i)

    def eval(self, tokens: Sequence[int], n_threads: int = 6) -> np.ndarray:
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.full(self.n_embd, np.nan, dtype=np.float32)
        self.lib.bert_eval(self.ctx, n_threads, _i32p(toks), len(toks), _f32p(out))
        return out

    def eval_batch(self, sentences: Sequence[Sequence[int]], n_threads: int = 6, scattered: bool = False) -> np.ndarray:
        """bert_eval_batch through per-sentence host pointers, exactly like a C caller.  scattered: the result rows are
        every other row of a wider matrix (rows that are NOT the rows of one [B][n_embd] matrix)."""
        B = len(sentences)
        arrs = [np.ascontiguousarray(s, dtype=np.int32) for s in sentences]
        wide = np.full((B, 2 * self.n_embd + 3 if scattered else self.n_embd), np.nan, dtype=np.float32)
        out = wide[:, : self.n_embd]
        tok_ptrs = (C.POINTER(C.c_int32) * B)(*[_i32p(a) for a in arrs])
        lens = np.array([len(a) for a in arrs], dtype=np.int32)
        out_ptrs = (C.POINTER(C.c_float) * B)(*[C.cast(wide[i].ctypes.data, C.POINTER(C.c_float)) for i in range(B)])
        self.lib.bert_eval_batch(self.ctx, n_threads, B, tok_ptrs, _i32p(lens), out_ptrs)
        if scattered:
            assert np.isnan(wide[:, self.n_embd:]).all()          # nothing written beside the rows
        return np.ascontiguousarray(out)

    def encode(self, text: str, n_threads: int = 6) -> np.ndarray:
        out = np.full(self.n_embd, np.nan, dtype=np.float32)
        self.lib.bert_encode(self.ctx, n_threads, text.encode("utf-8"), _f32p(out))
        return out

    def encode_batch(self, texts: Sequence[str], n_threads: int = 6, batch_size: int = 16) -> np.ndarray:
        n = len(texts)
        out = np.full((n, self.n_embd), np.nan, dtype=np.float32)
        out_ptrs = (C.POINTER(C.c_float) * n)(*[_f32p(out[i]) for i in range(n)])
        txt = (C.c_char_p * n)(*[t.encode("utf-8") for t in texts])
        self.lib.bert_encode_batch(self.ctx, n_threads, batch_size, n, txt, out_ptrs)
        return out

    # ---- bert_hip.h -----------------------------------------------------------------------
    def eval_packed(self, tokens: np.ndarray, cu_seqlens: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """out: the caller's result rows, as in the C ABI (bert.h: `float **batch_embeddings`); a fresh NaN-filled array if None."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        B = len(cu) - 1
        if out is None:
            out = np.full((B, self.n_embd), np.nan, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (B, self.n_embd)
        r = self.lib.bert_hip_eval_packed(self.ctx, _i32p(tokens), _i32p(cu), B, _f32p(out))
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed failed: {r}")
        return out

    def n_devices(self) -> int:
        return self.lib.bert_hip_n_devices(self.ctx)

    @property
    def relative_attention(self) -> bool:
        """The model file holds MPNet's relative position bias (encoder.relative_attention_bias.weight); tokenizer-only contexts too."""
        return self.lib.bert_hip_relative_attention(self.ctx) == 1

    # ---- sentence pairs and scores --------------------------------------------------------
    @property
    def n_labels(self) -> int:
        """Labels of the model's classification head, 0 without one."""
        return self.lib.bert_hip_n_labels(self.ctx)

    def tokenize_pair(self, a: str | bytes, b: str | bytes, n_max_tokens: Optional[int] = None):
        """(ids, first_len) of [CLS] a [SEP] b [SEP], cut to n_max_tokens (tokenizer-only contexts too)."""
        n_max = n_max_tokens or self.n_max_tokens
        buf = np.zeros(max(n_max, 4), dtype=np.int32)
        n, fl = C.c_int32(0), C.c_int32(0)
        da, db = (t if isinstance(t, bytes) else t.encode("utf-8") for t in (a, b))
        r = self.lib.bert_hip_tokenize_pair(self.ctx, da, db, _i32p(buf), C.byref(n), C.byref(fl), n_max)
        if r != 0:
            raise RuntimeError(f"bert_hip_tokenize_pair failed: {r}")
        return buf[: n.value].tolist(), fl.value

    def eval_packed_typed(self, tokens: np.ndarray, cu_seqlens: np.ndarray, first_len=None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """eval_packed with token types: first_len[b] leading tokens of sentence b take type 0, the rest type 1 (None: all type 0)."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        fl = None if first_len is None else np.ascontiguousarray(first_len, dtype=np.int32)
        B = len(cu) - 1
        if out is None:
            out = np.full((B, self.n_embd), np.nan, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (B, self.n_embd) and (fl is None or len(fl) == B)
        r = self.lib.bert_hip_eval_packed_typed(self.ctx, _i32p(tokens), _i32p(cu), None if fl is None else _i32p(fl), B, _f32p(out))
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_typed failed: {r}")
        return out

    def eval_packed_typed_device(self, d_tokens_ptr: int, d_cu_ptr: int, d_first_len_ptr: Optional[int], n_sentences: int, n_tokens: int,
                                 max_len: int, d_out_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_eval_packed_typed_device(self.ctx, d_tokens_ptr, d_cu_ptr, d_first_len_ptr, n_sentences, n_tokens, max_len, d_out_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_typed_device failed: {r}")

    def score_packed(self, tokens: np.ndarray, cu_seqlens: np.ndarray, first_len=None, sigmoid: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Cross-encoder scores [B, n_labels] of a packed, typed batch: the logits, or 1 / (1 + exp(-logit)) with sigmoid."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        fl = None if first_len is None else np.ascontiguousarray(first_len, dtype=np.int32)
        B = len(cu) - 1
        if out is None:
            out = np.full((B, max(self.n_labels, 1)), np.nan, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and (fl is None or len(fl) == B)
        r = self.lib.bert_hip_score_packed(self.ctx, _i32p(tokens), _i32p(cu), None if fl is None else _i32p(fl), B, int(sigmoid), _f32p(out))
        if r != 0:
            raise RuntimeError(f"bert_hip_score_packed failed: {r}")
        return out

    def score_packed_device(self, d_tokens_ptr: int, d_cu_ptr: int, d_first_len_ptr: Optional[int], n_sentences: int, n_tokens: int, max_len: int,
                            d_scores_ptr: int, sigmoid: bool = False, stream: int = 0) -> None:
        r = self.lib.bert_hip_score_packed_device(self.ctx, d_tokens_ptr, d_cu_ptr, d_first_len_ptr, n_sentences, n_tokens, max_len, int(sigmoid),
                                                  d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_score_packed_device failed: {r}")

    def score_pairs(self, pairs: Sequence, sigmoid: bool = False, n_threads: int = 6) -> np.ndarray:
        """Scores [n, n_labels] of (a, b) text pairs: tokenize_pair at the model's n_max_tokens, then score_packed."""
        n = len(pairs)
        enc = lambda t: t if isinstance(t, bytes) else t.encode("utf-8")
        ta = (C.c_char_p * n)(*[enc(p[0]) for p in pairs])
        tb = (C.c_char_p * n)(*[enc(p[1]) for p in pairs])
        out = np.full((n, max(self.n_labels, 1)), np.nan, dtype=np.float32)
        r = self.lib.bert_hip_score_pairs(self.ctx, n_threads, n, ta, tb, int(sigmoid), _f32p(out))
        if r != n:
            raise RuntimeError(f"bert_hip_score_pairs scored {r} of {n} pairs")
        return out

    def rerank(self, query: str | bytes, docs: Sequence, top_k: Optional[int] = None):
        """(order, scores): the documents' indices by the first label's score, descending, ties by index; the scores in that order."""
        s = self.score_pairs([(query, d) for d in docs])[:, 0] if len(docs) else np.zeros(0, dtype=np.float32)
        order = np.argsort(-s, kind="stable")
        if top_k is not None:
            order = order[:top_k]
        return order, s[order]

    # ---- learned sparse embeddings --------------------------------------------------------
    @property
    def has_mlm_head(self) -> bool:
        """Whether the model file carries a masked-language-model head."""
        return bool(self.lib.bert_hip_has_mlm_head(self.ctx))

    def sparse_packed(self, tokens: np.ndarray, cu_seqlens: np.ndarray, k: Optional[int] = None, out=None):
        """Learned sparse weights of a packed batch: float32 [B, n_vocab], or with k (ids int32 [B, k], weights float32 [B, k]) — the k
        largest positive weights, larger first, equal weights smaller id first, unused places id -1 / weight 0.  out: the array(s) to fill."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        B = len(cu) - 1
        if k is None:
            w = np.full((B, self.n_vocab), np.nan, dtype=np.float32) if out is None else out
            assert w.dtype == np.float32 and w.flags.c_contiguous and w.shape == (B, self.n_vocab)
            r = self.lib.bert_hip_sparse_packed(self.ctx, _i32p(tokens), _i32p(cu), B, _f32p(w))
            if r != 0:
                raise RuntimeError(f"bert_hip_sparse_packed failed: {r}")
            return w
        ids, w = (np.full((B, max(k, 1)), -1, dtype=np.int32), np.zeros((B, max(k, 1)), dtype=np.float32)) if out is None else out
        assert ids.dtype == np.int32 and w.dtype == np.float32 and ids.flags.c_contiguous and w.flags.c_contiguous
        r = self.lib.bert_hip_sparse_topk_packed(self.ctx, _i32p(tokens), _i32p(cu), B, k, _i32p(ids), _f32p(w))
        if r != 0:
            raise RuntimeError(f"bert_hip_sparse_topk_packed failed: {r}")
        return ids, w

    def sparse_packed_device(self, d_tokens_ptr: int, d_cu_ptr: int, n_sentences: int, n_tokens: int, max_len: int, d_weights_ptr: int,
                             k: Optional[int] = None, d_ids_ptr: Optional[int] = None, stream: int = 0) -> None:
        if k is None:
            r = self.lib.bert_hip_sparse_packed_device(self.ctx, d_tokens_ptr, d_cu_ptr, n_sentences, n_tokens, max_len, d_weights_ptr, stream)
        else:
            r = self.lib.bert_hip_sparse_topk_packed_device(self.ctx, d_tokens_ptr, d_cu_ptr, n_sentences, n_tokens, max_len, k, d_ids_ptr, d_weights_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_sparse{'' if k is None else '_topk'}_packed_device failed: {r}")

    def encode_sparse(self, texts: Sequence, k: Optional[int] = None, n_threads: int = 6):
        """Learned sparse embeddings of texts: dense float32 [n, n_vocab], or (ids, weights) of the k largest terms when k is given."""
        n = len(texts)
        if k is None:
            toks = self.tokenize_batch(texts, n_threads)
            cu = np.concatenate([[0], np.cumsum([len(t) for t in toks])]).astype(np.int32)
            return self.sparse_packed(np.concatenate(toks).astype(np.int32) if n else np.zeros(0, np.int32), cu)
        arr = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        ids = np.full((n, max(k, 1)), -1, dtype=np.int32)
        w = np.zeros((n, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_encode_sparse_batch(self.ctx, n_threads, n, arr, k, _i32p(ids), _f32p(w))
        if r != n:
            raise RuntimeError(f"bert_hip_encode_sparse_batch encoded {r} of {n} texts")
        return ids, w

    # ---- long texts -----------------------------------------------------------------------
    def tokenize_long(self, text: str | bytes) -> List[int]:
        """All ids of a text, [CLS] ... [SEP], without truncation (tokenizer-only contexts too)."""
        data = text if isinstance(text, bytes) else text.encode("utf-8")
        n = self.lib.bert_hip_tokenize_long(self.ctx, data, None, 0)
        if n < 0:
            raise RuntimeError(f"bert_hip_tokenize_long failed: {n}")
        ids = np.zeros(n, dtype=np.int32)
        assert self.lib.bert_hip_tokenize_long(self.ctx, data, _i32p(ids), n) == n
        return ids.tolist()

    def plan_windows(self, n_tokens: int, window: Optional[int] = None, stride: Optional[int] = None) -> List[int]:
        window, stride = self.long_defaults(window, stride)
        return plan_windows(n_tokens, window, stride)

    def long_defaults(self, window: Optional[int] = None, stride: Optional[int] = None):
        """window: 128 ids (one full window of the one-launch kernel) where the model has the positions, else n_max_tokens; stride: three
        quarters of the window's inner length."""
        if window is None:
            window = min(self.n_max_tokens, 128)
        if stride is None:
            stride = max(1, 3 * (window - 2) // 4)
        return int(window), int(stride)

    def eval_packed_grouped(self, tokens: np.ndarray, cu_seqlens: np.ndarray, group_cu: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """One embedding per group of consecutive sentences (bert_hip_eval_packed_grouped); out: the caller's [n_groups, n_embd] rows, NaNs
        if None.  Raises ValueError for a group_cu the entry refuses (-2: out untouched)."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        g = np.ascontiguousarray(group_cu, dtype=np.int32)
        if out is None:
            out = np.full((len(g) - 1, self.n_embd), np.nan, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (len(g) - 1, self.n_embd)
        r = self.lib.bert_hip_eval_packed_grouped(self.ctx, _i32p(tokens), _i32p(cu), len(cu) - 1, _i32p(g), len(g) - 1, _f32p(out))
        if r == -2:
            raise ValueError("bert_hip_eval_packed_grouped refused its arguments (see stderr)")
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_grouped failed: {r}")
        return out

    def eval_packed_grouped_device(self, d_tokens_ptr: int, d_cu_ptr: int, n_sentences: int, n_tokens: int, max_len: int, d_group_cu_ptr: int,
                                   n_groups: int, d_out_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_eval_packed_grouped_device(self.ctx, d_tokens_ptr, d_cu_ptr, n_sentences, n_tokens, max_len, d_group_cu_ptr,
                                                         n_groups, d_out_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_grouped_device failed: {r}")

    def encode_long_batch(self, texts: Sequence[str], window: Optional[int] = None, stride: Optional[int] = None, n_threads: int = 6,
                          return_windows: bool = False):
        """One embedding per text of any length (bert_hip_encode_long_batch); return_windows: also the number of windows per text.
        Raises ValueError for a window or stride the entry refuses."""
        window, stride = self.long_defaults(window, stride)
        n = len(texts)
        out = np.full((n, self.n_embd), np.nan, dtype=np.float32)
        out_ptrs = (C.POINTER(C.c_float) * n)(*[_f32p(out[i]) for i in range(n)])
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        nw = np.full(n, -1, dtype=np.int32)
        r = self.lib.bert_hip_encode_long_batch(self.ctx, n_threads, n, txt, window, stride, out_ptrs, _i32p(nw))
        if r == -2:
            raise ValueError(f"bert_hip_encode_long_batch refused window {window}, stride {stride}")
        if r != n:
            raise RuntimeError(f"bert_hip_encode_long_batch encoded {r} of {n} texts")
        return (out, nw) if return_windows else out

    # ---- token rows and late interaction ---------------------------------------------------
    def eval_packed_tokens(self, tokens: np.ndarray, cu_seqlens: np.ndarray, normalize: bool = True, with_embeddings: bool = False):
        """The final state of every token of a packed batch (bert_hip_eval_packed_tokens): rows [n_tokens, n_embd] f32, each over its L2
        norm if normalize; with_embeddings: (rows, embeddings [n_sentences, n_embd]), the embeddings eval_packed's bits."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        B = len(cu) - 1
        rows = np.full((int(cu[-1]), self.n_embd), np.nan, dtype=np.float32)
        emb = np.full((B, self.n_embd), np.nan, dtype=np.float32) if with_embeddings else None
        r = self.lib.bert_hip_eval_packed_tokens(self.ctx, _i32p(tokens), _i32p(cu), B, int(bool(normalize)), _f32p(rows),
                                                 _f32p(emb) if with_embeddings else None)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_tokens failed: {r}")
        return (rows, emb) if with_embeddings else rows

    def eval_packed_tokens_device(self, d_tokens_ptr: int, d_cu_ptr: int, n_sentences: int, n_tokens: int, max_len: int, d_rows_ptr: int,
                                  d_embeddings_ptr: Optional[int] = None, normalize: bool = True, f16: bool = False, stream: int = 0) -> None:
        r = self.lib.bert_hip_eval_packed_tokens_device(self.ctx, d_tokens_ptr, d_cu_ptr, n_sentences, n_tokens, max_len,
                                                        int(bool(normalize)) | 2 * int(bool(f16)), d_rows_ptr, d_embeddings_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_tokens_device failed: {r}")

    def encode_tokens(self, texts: Sequence[str], normalize: bool = True, n_threads: int = 6):
        """Token rows of texts (bert_hip_encode_tokens_batch; tokenized and truncated as encode_batch does): (rows [n_tokens, n_embd] f32,
        cu [n_texts + 1] int32)."""
        n = len(texts)
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        cu = np.zeros(n + 1, dtype=np.int32)
        flags = int(bool(normalize))
        total = self.lib.bert_hip_encode_tokens_batch(self.ctx, n_threads, n, txt, flags, _i32p(cu), None, 0)
        if total < 0:
            raise RuntimeError(f"bert_hip_encode_tokens_batch failed: {total}")
        rows = np.full((total, self.n_embd), np.nan, dtype=np.float32)
        if self.lib.bert_hip_encode_tokens_batch(self.ctx, n_threads, n, txt, flags, _i32p(cu), _f32p(rows), total) != total:
            raise RuntimeError("bert_hip_encode_tokens_batch failed")
        return rows, cu

    def maxsim(self, q_rows, q_cu, d_rows, d_cu, pairs=None, mean: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
        """MaxSim of two packed sets of token rows (bert_hip_maxsim: f32 rows, rounded to f16 on the device): scores [n_q, n_d], or
        [n_pairs] for pairs [n_pairs, 2] of (query sentence, document sentence).  Raises ValueError for arguments the entry refuses
        (-2: out, if given, untouched)."""
        q = np.ascontiguousarray(q_rows, dtype=np.float32); d = np.ascontiguousarray(d_rows, dtype=np.float32)
        qcu = np.ascontiguousarray(q_cu, dtype=np.int32); dcu = np.ascontiguousarray(d_cu, dtype=np.int32)
        assert q.ndim == 2 and d.ndim == 2 and q.shape[1] == d.shape[1]
        n_q, n_d = len(qcu) - 1, len(dcu) - 1
        pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        if out is None:
            out = np.full(len(pr) if pr is not None else (n_q, n_d), np.nan, dtype=np.float32)
        r = self.lib.bert_hip_maxsim(self.ctx, _f32p(q), _i32p(qcu), n_q, _f32p(d), _i32p(dcu), n_d, q.shape[1], None if pr is None else _i32p(pr),
                                     0 if pr is None else len(pr), int(bool(mean)), _f32p(out))
        if r == -2:
            raise ValueError("bert_hip_maxsim refused its arguments (see stderr)")
        if r != 0:
            raise RuntimeError(f"bert_hip_maxsim failed: {r}")
        return out

    def maxsim_device(self, d_q_ptr: int, d_qcu_ptr: int, n_q: int, d_d_ptr: int, d_dcu_ptr: int, n_d: int, H: int, d_pairs_ptr: Optional[int],
                      n_pairs: int, d_scores_ptr: int, mean: bool = False, stream: int = 0) -> None:
        """bert_hip_maxsim_device: f16 rows, lengths, pairs (or None) and scores in device memory, enqueued on stream."""
        r = self.lib.bert_hip_maxsim_device(self.ctx, d_q_ptr, d_qcu_ptr, n_q, d_d_ptr, d_dcu_ptr, n_d, H, d_pairs_ptr, n_pairs, int(bool(mean)),
                                            d_scores_ptr, stream)
        if r == -2:
            raise ValueError("bert_hip_maxsim_device refused its arguments (see stderr)")
        if r != 0:
            raise RuntimeError(f"bert_hip_maxsim_device failed: {r}")

    def eval_packed_gather(self, tokens: np.ndarray, cu_seqlens: np.ndarray) -> List[int]:
        """Evaluates on all devices of the context and gathers on every device: returns the device pointers of the
        [n_sentences][n_embd] f32 matrices, one per device (owned by the context)."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
        ptrs = (C.c_void_p * self.n_devices())()
        r = self.lib.bert_hip_eval_packed_gather(self.ctx, _i32p(tokens), _i32p(cu), len(cu) - 1, ptrs)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_gather failed: {r}")
        return [int(p) for p in ptrs]

    def reserve(self, n_tokens: int, n_sentences: int) -> None:
        if self.lib.bert_hip_reserve(self.ctx, n_tokens, n_sentences) != 0:
            raise RuntimeError("bert_hip_reserve failed")

    def check(self) -> int:
        return self.lib.bert_hip_check(self.ctx)

    def encode_batch_count(self, texts: Sequence[str], n_threads: int = 6):
        n = len(texts)
        out = np.full((n, self.n_embd), np.nan, dtype=np.float32)
        out_ptrs = (C.POINTER(C.c_float) * n)(*[_f32p(out[i]) for i in range(n)])
        txt = (C.c_char_p * n)(*[t.encode("utf-8") for t in texts])
        return self.lib.bert_hip_encode_batch(self.ctx, n_threads, n, txt, out_ptrs), out

    def eval_packed_device(self, d_tokens_ptr: int, d_cu_ptr: int, n_sentences: int, n_tokens: int, max_len: int,
                           d_out_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_eval_packed_device(self.ctx, d_tokens_ptr, d_cu_ptr, n_sentences, n_tokens, max_len,
                                                 d_out_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_packed_device failed: {r}")

    def eval_hidden(self, tokens: Sequence[int]):
        toks = np.ascontiguousarray(tokens, dtype=np.int32)
        hid = np.empty((self.n_layer + 1, len(toks), self.n_embd), dtype=np.float32)
        out = np.empty(self.n_embd, dtype=np.float32)
        r = self.lib.bert_hip_eval_hidden(self.ctx, _i32p(toks), len(toks), _f32p(hid), _f32p(out))
        if r != 0:
            raise RuntimeError(f"bert_hip_eval_hidden failed: {r}")
        return out, hid

    def profile(self, on: bool) -> None:
        self.lib.bert_hip_profile_enable(self.ctx, int(on))

    def profile_report(self, families: bool = False) -> dict:
        """{kernel: {launches, total_ms, flops_per_launch}}; families=True adds the "family:<kernel>_<weights>" lines (which
        mat-mul kernel served the launches: gemm256_f16 / gemm256_q4 / gemm_mfma_f16 / gemm_mfma_q4 / gemm_naive)."""
        buf = C.create_string_buffer(1 << 16)
        self.lib.bert_hip_profile_report(self.ctx, buf, len(buf))
        out = {}
        for line in buf.value.decode().splitlines():
            name, launches, ms, flops = line.split()
            if families or not name.startswith("family:"):
                out[name] = {"launches": int(launches), "total_ms": float(ms), "flops_per_launch": float(flops)}
        return out

    def set_option(self, key: str, value: str) -> None:
        self.lib.bert_hip_set_option(self.ctx, key.encode(), value.encode())

    def pooling(self) -> int:
        """0 mean, 1 cls (set_option "pooling" / BERT_HIP_POOLING); -1 for a tokenizer-only context."""
        return int(self.lib.bert_hip_pooling(self.ctx))

    def normalize(self) -> int:
        """1 or 0 (set_option "normalize" / BERT_HIP_NORMALIZE); -1 for a tokenizer-only context."""
        return int(self.lib.bert_hip_normalize(self.ctx))

    def index(self, dim: Optional[int] = None, dtype: str = "f16") -> "BertIndex":
        """An embedding index on the context's first device (bert_hip_index_create): dim None = n_embd, dtype "f16" | "f32" |
        "i8" (one int8 code per element and one f32 scale per row) | "b1" (one sign bit per element, searched with int8
        queries: the coarse stage of BertIndex.search_rescored)."""
        return BertIndex(self, dim, dtype)

    def sparse_index(self, width: int = 128, dtype: str = "f32", n_vocab: Optional[int] = None) -> "BertSparseIndex":
        """A sparse index on the context's first device (bert_hip_sparse_index_create): rows of at most width (id, weight) terms, dtype
        "f32" (i32 ids, f32 weights) | "f16" (u16 ids, f16 weights; n_vocab <= 65536); n_vocab None = the model's."""
        return BertSparseIndex(self, width, dtype, n_vocab)

    def token_index(self, dim: Optional[int] = None, dtype: str = "f16") -> "BertTokenIndex":
        """A token index on the context's first device (bert_hip_token_index_create): documents' f16 token rows, exact MaxSim top-k
        search; dim None = n_embd.  dtype "i8": int8 codes with a scale per token (bert_hip_late_index_create)."""
        return BertTokenIndex(self, dim, dtype=dtype)

    def load_index(self, path: str) -> "BertIndex":
        """The index a BertIndex.save wrote (bert_hip_index_load), on this context's first device."""
        return BertIndex(self, _load=path)

    def load_sparse_index(self, path: str) -> "BertSparseIndex":
        """The sparse index a BertSparseIndex.save wrote (bert_hip_sparse_index_load), on this context's first device."""
        return BertSparseIndex(self, _load=path)

    def load_token_index(self, path: str) -> "BertTokenIndex":
        """The token index a BertTokenIndex.save wrote (bert_hip_late_index_load), on this context's first device."""
        return BertTokenIndex(self, _load=path)


def allow_words(allow, n_rows: int) -> np.ndarray:
    """An allow-list as the uint32 words of bert_hip_index_search_filtered: a bool array of n_rows entries is packed (row 32 w + b
    = bit b of word w), uint32 words pass through."""
    a = np.asarray(allow)
    if a.dtype == np.uint32:
        return np.ascontiguousarray(a).reshape(-1)
    if a.dtype != np.bool_ or a.shape != (n_rows,):
        raise ValueError(f"allow must be a bool array of {n_rows} entries or uint32 words")
    packed = np.packbits(a, bitorder="little").tobytes().ljust((n_rows + 31) // 32 * 4, b"\0")
    return np.frombuffer(packed, dtype="<u4").astype(np.uint32)


class BertIndex:
    """bert_hip_index_*: rows in HBM, exact top-k inner-product search.  search* return (ids [n, k] int32, scores [n, k] f32),
    best first; missing entries are id -1, score -inf.  The *_device forms take device pointers (ints, e.g. torch's
    data_ptr()) and a stream handle, and return at once."""

    def __init__(self, model: BertModel, dim: Optional[int] = None, dtype: str = "f16", _load: Optional[str] = None):
        if dtype not in ("f16", "f32", "i8", "b1"):
            raise ValueError("dtype must be 'f16', 'f32', 'i8' or 'b1'")
        self.model, self.lib = model, model.lib
        if _load is not None:
            # dim and dtype come from the file's header (include/bert_hip.h: u32 dtype at byte 12, u32 dim at 16)
            self.ix = self.lib.bert_hip_index_load(model.ctx, os.fsencode(_load))
            if not self.ix:
                raise RuntimeError("bert_hip_index_load failed (see stderr)")
            with open(_load, "rb") as f:
                head = np.frombuffer(f.read(24), dtype="<u4")
            self.dtype, self.dim = ("f32", "f16", "i8", "b1")[int(head[3])], int(head[4])
            return
        code = {"f16": 1, "i8": 2, "b1": 3}.get(dtype, 0)
        self.ix = self.lib.bert_hip_index_create(model.ctx, 0 if dim is None else int(dim), code)
        if not self.ix:
            raise RuntimeError("bert_hip_index_create failed (see stderr)")
        self.dim = model.n_embd if dim is None else int(dim)
        self.dtype = dtype

    def close(self):
        # (an index the context freed already — bert_free frees its indexes — must not be freed again)
        if getattr(self, "ix", None) and getattr(self.model, "ctx", None):
            self.lib.bert_hip_index_free(self.ix)
        self.ix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self.lib.bert_hip_index_size(self.ix))

    def reserve(self, n_rows: int, n_queries: int = 0, k: int = 1) -> None:
        if self.lib.bert_hip_index_reserve(self.ix, n_rows, n_queries, k) != 0:
            raise RuntimeError("bert_hip_index_reserve failed")

    def add(self, rows) -> int:
        """rows [n, dim] (converted to f32); returns the first new id."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        r = self.lib.bert_hip_index_add(self.ix, rows.shape[0], _f32p(rows))
        if r < 0:
            raise RuntimeError(f"bert_hip_index_add failed: {r}")
        return r

    def add_device(self, n: int, d_rows_ptr: int, stream: int = 0) -> int:
        r = self.lib.bert_hip_index_add_device(self.ix, n, d_rows_ptr, stream)
        if r < 0:
            raise RuntimeError(f"bert_hip_index_add_device failed: {r}")
        return r

    def add_texts(self, texts: Sequence[str], n_threads: int = 6) -> int:
        n = len(texts)
        txt = (C.c_char_p * n)(*[t.encode("utf-8") for t in texts])
        r = self.lib.bert_hip_index_add_texts(self.ix, n_threads, n, txt)
        if r < 0:
            raise RuntimeError(f"bert_hip_index_add_texts failed: {r}")
        return r

    def add_long_texts(self, texts: Sequence[str], window: Optional[int] = None, stride: Optional[int] = None, n_threads: int = 6) -> int:
        """add_texts for texts of any length: one row per text (bert_hip_index_add_long_texts); returns the first new id.  Raises
        ValueError for a window or stride the entry refuses (the index keeps its size)."""
        window, stride = self.model.long_defaults(window, stride)
        n = len(texts)
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        r = self.lib.bert_hip_index_add_long_texts(self.ix, n_threads, n, txt, window, stride)
        if r == -2:
            raise ValueError(f"bert_hip_index_add_long_texts refused window {window}, stride {stride}")
        if r < 0:
            raise RuntimeError(f"bert_hip_index_add_long_texts failed: {r}")
        return r

    def search(self, queries, k: int = 10, allow=None):
        """allow: None, a bool array of len(index) entries (True = the row may be returned), or uint32 words (bit b of word w =
        row 32 w + b), which are passed through."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        if allow is None:
            r = self.lib.bert_hip_index_search(self.ix, q.shape[0], _f32p(q), k, _i32p(ids), _f32p(scores))
            if r != 0:
                raise RuntimeError(f"bert_hip_index_search failed: {r}")
            return ids, scores
        words = allow_words(allow, len(self))
        r = self.lib.bert_hip_index_search_filtered(self.ix, q.shape[0], _f32p(q), k, words.ctypes.data, len(words), _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_filtered failed: {r}")
        return ids, scores

    def search_device(self, n_queries: int, d_queries_ptr: int, k: int, d_ids_ptr: int, d_scores_ptr: int, stream: int = 0,
                      d_allow_ptr: Optional[int] = None, n_words: int = 0) -> None:
        if d_allow_ptr is None:
            r = self.lib.bert_hip_index_search_device(self.ix, n_queries, d_queries_ptr, k, d_ids_ptr, d_scores_ptr, stream)
            if r != 0:
                raise RuntimeError(f"bert_hip_index_search_device failed: {r}")
            return
        r = self.lib.bert_hip_index_search_filtered_device(self.ix, n_queries, d_queries_ptr, k, d_allow_ptr, n_words, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_filtered_device failed: {r}")

    def rescore(self, queries, cand_ids, k: int = 10):
        """bert_hip_index_rescore: the best k of each query's own candidates, cand_ids [n_queries, n_cand] int32 (-1 and removed
        rows are skipped; ids outside [-1, len(index)) are an error), scored by this index's rule."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        cand = np.ascontiguousarray(cand_ids, dtype=np.int32).reshape(q.shape[0], -1)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        r = self.lib.bert_hip_index_rescore(self.ix, q.shape[0], _f32p(q), cand.shape[1], _i32p(cand), k, _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_rescore failed: {r}")
        return ids, scores

    def rescore_device(self, n_queries: int, d_queries_ptr: int, n_cand: int, d_cand_ptr: int, k: int, d_ids_ptr: int,
                       d_scores_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_index_rescore_device(self.ix, n_queries, d_queries_ptr, n_cand, d_cand_ptr, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_index_rescore_device failed: {r}")

    def search_rescored(self, fine: "BertIndex", queries, k: int = 10, n_cand: int = 100):
        """Two-stage search (bert_hip_index_search_rescored): this index (a "b1" one, say) picks n_cand candidates per query,
        `fine` — an index of the same rows — rescores them and returns its best k."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        r = self.lib.bert_hip_index_search_rescored(self.ix, fine.ix, q.shape[0], _f32p(q), n_cand, k, _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_rescored failed: {r}")
        return ids, scores

    def search_rescored_device(self, fine: "BertIndex", n_queries: int, d_queries_ptr: int, n_cand: int, k: int, d_ids_ptr: int,
                               d_scores_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_index_search_rescored_device(self.ix, fine.ix, n_queries, d_queries_ptr, n_cand, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_rescored_device failed: {r}")

    def get_rows(self, ids) -> np.ndarray:
        """bert_hip_index_get_rows: the stored rows `ids` as f32 [n, dim], removed rows included."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        rows = np.empty((len(ids), self.dim), dtype=np.float32)
        r = self.lib.bert_hip_index_get_rows(self.ix, len(ids), _i32p(ids), _f32p(rows))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_get_rows failed: {r}")
        return rows

    def kmeans(self, n_lists: int, n_iter: int, centroids) -> np.ndarray:
        """bert_hip_index_kmeans: n_iter steps of spherical k-means over the live rows from the initial centroids [n_lists, dim];
        returns the refined centroids.  The index is unchanged."""
        c = np.array(centroids, dtype=np.float32, order="C").reshape(n_lists, self.dim)
        r = self.lib.bert_hip_index_kmeans(self.ix, n_lists, n_iter, _f32p(c))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_kmeans failed: {r}")
        return c

    def partition(self, centroids) -> None:
        """bert_hip_index_partition: installs centroids [n_lists, dim] and assigns every current row to its nearest one; None or
        an empty array drops the partition."""
        c = np.zeros((0, self.dim), np.float32) if centroids is None else np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, self.dim)
        r = self.lib.bert_hip_index_partition(self.ix, c.shape[0], _f32p(c))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_partition failed: {r}")

    @property
    def n_lists(self) -> int:
        """the number of lists of the partition, 0 without one"""
        return int(self.lib.bert_hip_index_n_lists(self.ix))

    def centroids(self) -> np.ndarray:
        """the partition's centroids [n_lists, dim] as installed"""
        c = np.empty((max(self.n_lists, 0), self.dim), dtype=np.float32)
        r = self.lib.bert_hip_index_partition_centroids(self.ix, _f32p(c))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_partition_centroids failed: {r}")
        return c

    def partition_lists(self) -> np.ndarray:
        """the list of every row [len(index)] int32, -1 for the rows added since partition (the tail)"""
        lists = np.empty(len(self), dtype=np.int32)
        r = self.lib.bert_hip_index_partition_lists(self.ix, _i32p(lists))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_partition_lists failed: {r}")
        return lists

    def live_ids(self) -> np.ndarray:
        """The ids a search can return, ascending.  With removed rows: found by rescoring every id against a zero query, 256
        candidates per query (a removed row is skipped, every other finite row scores 0)."""
        n = len(self)
        if self.n_live == n:
            return np.arange(n, dtype=np.int32)
        cand = np.full((n + 255) // 256 * 256, -1, np.int32)
        cand[:n] = np.arange(n, dtype=np.int32)
        ids, _ = self.rescore(np.zeros((len(cand) // 256, self.dim), np.float32), cand.reshape(-1, 256), 256)
        return np.sort(ids[ids >= 0])

    def train_partition(self, n_lists: int, n_iter: int = 10, seed: int = 0) -> np.ndarray:
        """Seeds the centroids with get_rows(numpy.random.default_rng(seed).choice(live_ids(), n_lists, replace=False)), refines
        them with kmeans(n_lists, n_iter) and installs them with partition; returns the centroids."""
        pick = np.random.default_rng(seed).choice(self.live_ids(), n_lists, replace=False)
        c = self.kmeans(n_lists, n_iter, self.get_rows(pick))
        self.partition(c)
        return c

    def search_probed(self, queries, k: int = 10, nprobe: int = 8, allow=None):
        """bert_hip_index_search_probed: the search over the rows of each query's nprobe nearest lists and the tail.  allow: as
        in search (bert_hip_index_search_probed_filtered)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        if allow is None:
            r = self.lib.bert_hip_index_search_probed(self.ix, q.shape[0], _f32p(q), nprobe, k, _i32p(ids), _f32p(scores))
            if r != 0:
                raise RuntimeError(f"bert_hip_index_search_probed failed: {r}")
            return ids, scores
        words = allow_words(allow, len(self))
        r = self.lib.bert_hip_index_search_probed_filtered(self.ix, q.shape[0], _f32p(q), nprobe, k, words.ctypes.data, len(words),
                                                           _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_probed_filtered failed: {r}")
        return ids, scores

    def search_probed_device(self, n_queries: int, d_queries_ptr: int, nprobe: int, k: int, d_ids_ptr: int, d_scores_ptr: int,
                             stream: int = 0, d_allow_ptr: int = 0, n_words: int = 0) -> None:
        if not d_allow_ptr:
            r = self.lib.bert_hip_index_search_probed_device(self.ix, n_queries, d_queries_ptr, nprobe, k, d_ids_ptr, d_scores_ptr, stream)
            if r != 0:
                raise RuntimeError(f"bert_hip_index_search_probed_device failed: {r}")
            return
        r = self.lib.bert_hip_index_search_probed_filtered_device(self.ix, n_queries, d_queries_ptr, nprobe, k, d_allow_ptr, n_words,
                                                                  d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_probed_filtered_device failed: {r}")

    def search_rescored_probed(self, fine: "BertIndex", queries, k: int = 10, n_cand: int = 100, nprobe: int = 8, allow=None):
        """Two-stage search over a partition (bert_hip_index_search_rescored_probed): this index's search_probed(k = n_cand,
        nprobe, allow) picks the candidates, which stay on the device; `fine` rescores them and returns its best k."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        ids = np.empty((q.shape[0], k), dtype=np.int32)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        words = None if allow is None else allow_words(allow, len(self))
        r = self.lib.bert_hip_index_search_rescored_probed(self.ix, fine.ix, q.shape[0], _f32p(q), nprobe, n_cand, k,
                                                           None if words is None else words.ctypes.data, 0 if words is None else len(words),
                                                           _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_rescored_probed failed: {r}")
        return ids, scores

    def search_rescored_probed_device(self, fine: "BertIndex", n_queries: int, d_queries_ptr: int, nprobe: int, n_cand: int, k: int,
                                      d_ids_ptr: int, d_scores_ptr: int, stream: int = 0, d_allow_ptr: int = 0, n_words: int = 0) -> None:
        r = self.lib.bert_hip_index_search_rescored_probed_device(self.ix, fine.ix, n_queries, d_queries_ptr, nprobe, n_cand, k,
                                                                  d_allow_ptr or None, n_words, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_rescored_probed_device failed: {r}")

    def save_partition(self, path: str) -> None:
        """bert_hip_index_partition_save: centroids, list ids and the tail's start, as a file of its own."""
        r = self.lib.bert_hip_index_partition_save(self.ix, os.fsencode(path))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_partition_save failed: {r}")

    def load_partition(self, path: str) -> None:
        """bert_hip_index_partition_load: installs the file's centroids and lists as they are (no assignment runs)."""
        r = self.lib.bert_hip_index_partition_load(self.ix, os.fsencode(path))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_partition_load failed: {r}")

    @property
    def n_live(self) -> int:
        return int(self.lib.bert_hip_index_n_live(self.ix))

    def remove(self, ids) -> int:
        """Marks rows as deleted (ids stay stable); returns the number newly removed."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        r = self.lib.bert_hip_index_remove(self.ix, len(ids), _i32p(ids))
        if r < 0:
            raise RuntimeError(f"bert_hip_index_remove failed: {r}")
        return r

    def compact(self) -> np.ndarray:
        """Drops the removed rows' storage; returns old_ids [n_live] int32: the former id of each new id."""
        old = np.empty(max(self.n_live, 0), dtype=np.int32)
        r = self.lib.bert_hip_index_compact(self.ix, _i32p(old))
        if r < 0:
            raise RuntimeError(f"bert_hip_index_compact failed: {r}")
        return old[:r]

    def save(self, path: str) -> None:
        r = self.lib.bert_hip_index_save(self.ix, os.fsencode(path))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_save failed: {r}")

    def search_texts(self, texts: Sequence[str], k: int = 10, n_threads: int = 6):
        n = len(texts)
        txt = (C.c_char_p * max(n, 1))(*[t.encode("utf-8") for t in texts])
        ids = np.empty((n, k), dtype=np.int32)
        scores = np.empty((n, k), dtype=np.float32)
        r = self.lib.bert_hip_index_search_texts(self.ix, n_threads, n, txt, k, _i32p(ids), _f32p(scores))
        if r != 0:
            raise RuntimeError(f"bert_hip_index_search_texts failed: {r}")
        return ids, scores

    # ---- hybrid search (bert_hip_hybrid_*): this index and a sparse index of the same rows, H = (w_dense * D) + (w_sparse * S)
    @staticmethod
    def _hybrid_fail(name: str, r: int):
        if r == -2:
            raise ValueError(f"{name} refused its arguments (see stderr)")
        raise RuntimeError(f"{name} failed: {r}")

    def hybrid_reserve(self, sparse: "BertSparseIndex", n_rows: int, n_queries: int = 0, k: int = 1) -> None:
        r = self.lib.bert_hip_hybrid_reserve(self.ix, sparse.ix, n_rows, n_queries, k)
        if r != 0:
            self._hybrid_fail("bert_hip_hybrid_reserve", r)

    def _hybrid_search(self, entry: str, sparse: "BertSparseIndex", queries, q_ids, q_weights, k, w_dense, w_sparse, allow):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        q_ids, q_weights = BertSparseIndex._terms(q_ids, q_weights)
        if q_ids.shape[0] != q.shape[0]:
            raise ValueError("the dense and the sparse queries differ in number")
        nq = q.shape[0]
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        words = None if allow is None else allow_words(allow, len(self))
        r = getattr(self.lib, entry)(self.ix, sparse.ix, nq, q.ctypes.data, q_ids.shape[1], q_ids.ctypes.data, q_weights.ctypes.data,
                                     w_dense, w_sparse, None if words is None else words.ctypes.data, 0 if words is None else len(words),
                                     k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._hybrid_fail(entry, r)
        return ids, scores

    def _hybrid_search_texts(self, entry: str, sparse: "BertSparseIndex", texts: Sequence, kq, k, w_dense, w_sparse, n_threads):
        n = len(texts)
        txt = (C.c_char_p * max(n, 1))(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        ids = np.empty((n, max(k, 1)), dtype=np.int32)
        scores = np.empty((n, max(k, 1)), dtype=np.float32)
        r = getattr(self.lib, entry)(self.ix, sparse.ix, n_threads, n, txt, kq, w_dense, w_sparse, k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._hybrid_fail(entry, r)
        return ids, scores

    def hybrid_search(self, sparse: "BertSparseIndex", queries, q_ids, q_weights, k: int = 10, w_dense: float = 1.0, w_sparse: float = 1.0,
                      allow=None):
        """The exact top-k of (w_dense * dense score) + (w_sparse * sparse score) over the rows live in both indexes and allowed:
        queries [n, dim] f32, (q_ids, q_weights) [n, kq] as BertSparseIndex.search takes them, allow as BertIndex.search's."""
        return self._hybrid_search("bert_hip_hybrid_search", sparse, queries, q_ids, q_weights, k, w_dense, w_sparse, allow)

    def hybrid_search_device(self, sparse: "BertSparseIndex", n_queries: int, d_queries_ptr: int, kq: int, d_q_ids_ptr: int, d_q_weights_ptr: int,
                             k: int, d_ids_ptr: int, d_scores_ptr: int, w_dense: float = 1.0, w_sparse: float = 1.0, stream: int = 0,
                             d_allow_ptr: int = 0, n_words: int = 0) -> None:
        r = self.lib.bert_hip_hybrid_search_device(self.ix, sparse.ix, n_queries, d_queries_ptr, kq, d_q_ids_ptr, d_q_weights_ptr, w_dense, w_sparse,
                                                   d_allow_ptr or None, n_words, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._hybrid_fail("bert_hip_hybrid_search_device", r)

    def hybrid_search_texts(self, sparse: "BertSparseIndex", texts: Sequence, kq: int = 32, k: int = 10, w_dense: float = 1.0, w_sparse: float = 1.0,
                            n_threads: int = 6):
        return self._hybrid_search_texts("bert_hip_hybrid_search_texts", sparse, texts, kq, k, w_dense, w_sparse, n_threads)

    # ---- the same searches over the sparse index's postings (bert_hip_dense_sparse_search_inverted*): the ids and score bits of the
    # three above; sparse.invert() must have covered every row, else a ValueError (-2)
    def hybrid_search_inverted(self, sparse: "BertSparseIndex", queries, q_ids, q_weights, k: int = 10, w_dense: float = 1.0,
                               w_sparse: float = 1.0, allow=None):
        """hybrid_search through the sparse index's postings: the same ids and score bits."""
        return self._hybrid_search("bert_hip_dense_sparse_search_inverted", sparse, queries, q_ids, q_weights, k, w_dense, w_sparse, allow)

    def hybrid_search_inverted_device(self, sparse: "BertSparseIndex", n_queries: int, d_queries_ptr: int, kq: int, d_q_ids_ptr: int,
                                      d_q_weights_ptr: int, k: int, d_ids_ptr: int, d_scores_ptr: int, w_dense: float = 1.0, w_sparse: float = 1.0,
                                      stream: int = 0, d_allow_ptr: int = 0, n_words: int = 0) -> None:
        r = self.lib.bert_hip_dense_sparse_search_inverted_device(self.ix, sparse.ix, n_queries, d_queries_ptr, kq, d_q_ids_ptr, d_q_weights_ptr,
                                                                  w_dense, w_sparse, d_allow_ptr or None, n_words, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._hybrid_fail("bert_hip_dense_sparse_search_inverted_device", r)

    def hybrid_search_inverted_texts(self, sparse: "BertSparseIndex", texts: Sequence, kq: int = 32, k: int = 10, w_dense: float = 1.0,
                                     w_sparse: float = 1.0, n_threads: int = 6):
        return self._hybrid_search_texts("bert_hip_dense_sparse_search_inverted_texts", sparse, texts, kq, k, w_dense, w_sparse, n_threads)


class BertSparseIndex:
    """bert_hip_sparse_index_*: rows of (vocabulary id, weight) terms in HBM, exact top-k inner-product search.  Rows and queries are
    (ids [n, kk] int32, weights [n, kk] float32) as BertModel.encode_sparse(texts, k) returns them, id -1 = unused place.  search*
    return (ids [n, k] int32, scores [n, k] f32), best first; missing entries are id -1, score -inf.  A ValueError is an argument the
    entry refused (-2).  The *_device forms take device pointers (ints) and a stream handle, and return at once."""

    def __init__(self, model: BertModel, width: int = 128, dtype: str = "f32", n_vocab: Optional[int] = None, _load: Optional[str] = None):
        if dtype not in ("f32", "f16"):
            raise ValueError("dtype must be 'f32' or 'f16'")
        self.model, self.lib = model, model.lib
        if _load is not None:
            # dtype, n_vocab and width come from the file's header (include/bert_hip.h: u32 dtype at byte 12, n_vocab at 16, width at 20)
            self.ix = self.lib.bert_hip_sparse_index_load(model.ctx, os.fsencode(_load))
            if not self.ix:
                raise RuntimeError("bert_hip_sparse_index_load failed (see stderr)")
            with open(_load, "rb") as f:
                head = np.frombuffer(f.read(24), dtype="<u4")
            self.dtype, self.n_vocab, self.width = ("f32", "f16")[int(head[3])], int(head[4]), int(head[5])
            return
        self.ix = self.lib.bert_hip_sparse_index_create(model.ctx, 0 if n_vocab is None else int(n_vocab), int(width), 1 if dtype == "f16" else 0)
        if not self.ix:
            raise RuntimeError("bert_hip_sparse_index_create failed (see stderr)")
        self.width, self.dtype = int(width), dtype
        self.n_vocab = model.n_vocab if n_vocab is None else int(n_vocab)

    def close(self):
        # (an index the context freed already — bert_free frees its indexes — must not be freed again)
        if getattr(self, "ix", None) and getattr(self.model, "ctx", None):
            self.lib.bert_hip_sparse_index_free(self.ix)
        self.ix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self.lib.bert_hip_sparse_index_size(self.ix))

    @staticmethod
    def _fail(name: str, r: int):
        if r == -2:
            raise ValueError(f"{name} refused its arguments (see stderr)")
        raise RuntimeError(f"{name} failed: {r}")

    @staticmethod
    def _terms(ids, weights):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if ids.ndim != 2 or ids.shape != weights.shape:
            raise ValueError("ids and weights must be 2-d arrays of one shape")
        return ids, weights

    def reserve(self, n_rows: int, n_queries: int = 0, k: int = 1) -> None:
        r = self.lib.bert_hip_sparse_index_reserve(self.ix, n_rows, n_queries, k)
        if r != 0:
            self._fail("bert_hip_sparse_index_reserve", r)

    def add(self, ids, weights) -> int:
        """rows (ids [n, k_in], weights [n, k_in]); returns the first new id."""
        ids, weights = self._terms(ids, weights)
        r = self.lib.bert_hip_sparse_index_add(self.ix, ids.shape[0], ids.shape[1], ids.ctypes.data, weights.ctypes.data)
        if r < 0:
            self._fail("bert_hip_sparse_index_add", r)
        return r

    def add_device(self, n: int, k_in: int, d_ids_ptr: int, d_weights_ptr: int, stream: int = 0) -> int:
        r = self.lib.bert_hip_sparse_index_add_device(self.ix, n, k_in, d_ids_ptr, d_weights_ptr, stream)
        if r < 0:
            self._fail("bert_hip_sparse_index_add_device", r)
        return r

    def add_texts(self, texts: Sequence, n_threads: int = 6) -> int:
        n = len(texts)
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        r = self.lib.bert_hip_sparse_index_add_texts(self.ix, n_threads, n, txt)
        if r < 0:
            self._fail("bert_hip_sparse_index_add_texts", r)
        return r

    def search(self, q_ids, q_weights, k: int = 10, allow=None):
        """allow: None, or the rows that may be returned — a bool array of len(index) entries or uint32 words (allow_words):
        bert_hip_sparse_index_search_filtered."""
        q_ids, q_weights = self._terms(q_ids, q_weights)
        nq = q_ids.shape[0]
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        if allow is None:
            name = "bert_hip_sparse_index_search"
            r = self.lib.bert_hip_sparse_index_search(self.ix, nq, q_ids.shape[1], q_ids.ctypes.data, q_weights.ctypes.data, k, ids.ctypes.data, scores.ctypes.data)
        else:
            name = "bert_hip_sparse_index_search_filtered"
            words = allow_words(allow, len(self))
            r = self.lib.bert_hip_sparse_index_search_filtered(self.ix, nq, q_ids.shape[1], q_ids.ctypes.data, q_weights.ctypes.data, k,
                                                               words.ctypes.data, len(words), ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail(name, r)
        return ids, scores

    def search_device(self, n_queries: int, kq: int, d_q_ids_ptr: int, d_q_weights_ptr: int, k: int, d_ids_ptr: int, d_scores_ptr: int,
                      stream: int = 0, d_allow_ptr: int = 0, n_words: int = 0) -> None:
        """d_allow_ptr: 0, or device uint32 words [n_words] as search's allow (bert_hip_sparse_index_search_filtered_device)."""
        if d_allow_ptr:
            name = "bert_hip_sparse_index_search_filtered_device"
            r = self.lib.bert_hip_sparse_index_search_filtered_device(self.ix, n_queries, kq, d_q_ids_ptr, d_q_weights_ptr, k, d_allow_ptr, n_words,
                                                                      d_ids_ptr, d_scores_ptr, stream)
        else:
            name = "bert_hip_sparse_index_search_device"
            r = self.lib.bert_hip_sparse_index_search_device(self.ix, n_queries, kq, d_q_ids_ptr, d_q_weights_ptr, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._fail(name, r)

    def rescore(self, q_ids, q_weights, cand_ids, k: int = 10):
        """bert_hip_sparse_index_rescore: per query its candidate rows cand_ids [n, n_cand] (-1 = none) scored with the search's bits,
        the best k of them."""
        q_ids, q_weights = self._terms(q_ids, q_weights)
        nq = q_ids.shape[0]
        cand = np.ascontiguousarray(cand_ids, dtype=np.int32).reshape(nq, -1)
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_sparse_index_rescore(self.ix, nq, q_ids.shape[1], q_ids.ctypes.data, q_weights.ctypes.data, cand.shape[1],
                                                   cand.ctypes.data, k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_sparse_index_rescore", r)
        return ids, scores

    def rescore_device(self, n_queries: int, kq: int, d_q_ids_ptr: int, d_q_weights_ptr: int, n_cand: int, d_cand_ptr: int, k: int,
                       d_ids_ptr: int, d_scores_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_sparse_index_rescore_device(self.ix, n_queries, kq, d_q_ids_ptr, d_q_weights_ptr, n_cand, d_cand_ptr, k,
                                                          d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._fail("bert_hip_sparse_index_rescore_device", r)

    def remove(self, ids) -> int:
        """bert_hip_sparse_index_remove: the number of rows newly removed."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        r = self.lib.bert_hip_sparse_index_remove(self.ix, len(ids), ids.ctypes.data)
        if r < 0:
            self._fail("bert_hip_sparse_index_remove", r)
        return r

    @property
    def n_live(self) -> int:
        return int(self.lib.bert_hip_sparse_index_n_live(self.ix))

    def compact(self) -> np.ndarray:
        """bert_hip_sparse_index_compact: drops the removed rows; returns the former ids of the rows now at 0 .. len(index) - 1."""
        old = np.empty(max(self.n_live, 1), dtype=np.int32)
        r = self.lib.bert_hip_sparse_index_compact(self.ix, old.ctypes.data)
        if r < 0:
            self._fail("bert_hip_sparse_index_compact", r)
        return old[:r]

    def save(self, path: str) -> None:
        r = self.lib.bert_hip_sparse_index_save(self.ix, os.fsencode(path))
        if r != 0:
            self._fail("bert_hip_sparse_index_save", r)

    def live_ids(self) -> np.ndarray:
        """The ids a search can return, ascending.  With removed rows: found by rescoring every id against an empty query, 256
        candidates per query (a removed row is skipped, every other row scores +0)."""
        n = len(self)
        if self.n_live == n:
            return np.arange(n, dtype=np.int32)
        cand = np.full((n + 255) // 256 * 256, -1, np.int32)
        cand[:n] = np.arange(n, dtype=np.int32)
        nq = len(cand) // 256
        ids, _ = self.rescore(np.full((nq, 1), -1, np.int32), np.zeros((nq, 1), np.float32), cand.reshape(-1, 256), 256)
        return np.sort(ids[ids >= 0])

    def search_texts(self, texts: Sequence, kq: int = 32, k: int = 10, n_threads: int = 6):
        n = len(texts)
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        ids = np.empty((n, max(k, 1)), dtype=np.int32)
        scores = np.empty((n, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_sparse_index_search_texts(self.ix, n_threads, n, txt, kq, k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_sparse_index_search_texts", r)
        return ids, scores

    def invert(self) -> int:
        """bert_hip_sparse_index_invert: builds the postings of all rows (the inverted searches read them); the rows covered."""
        r = self.lib.bert_hip_sparse_index_invert(self.ix)
        if r < 0:
            self._fail("bert_hip_sparse_index_invert", r)
        return r

    @property
    def inverted_rows(self) -> int:
        return int(self.lib.bert_hip_sparse_index_inverted_rows(self.ix))

    def search_inverted(self, q_ids, q_weights, k: int = 10, allow=None):
        """search through the postings (bert_hip_sparse_index_search_inverted): the ids and score bits of search(..., allow).  A
        ValueError too where the postings do not cover the rows (no invert yet, rows added since, compacted)."""
        q_ids, q_weights = self._terms(q_ids, q_weights)
        nq = q_ids.shape[0]
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        words = None if allow is None else allow_words(allow, len(self))
        r = self.lib.bert_hip_sparse_index_search_inverted(self.ix, nq, q_ids.shape[1], q_ids.ctypes.data, q_weights.ctypes.data, k,
                                                           None if words is None else words.ctypes.data, 0 if words is None else len(words),
                                                           ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_sparse_index_search_inverted", r)
        return ids, scores

    def search_inverted_device(self, n_queries: int, kq: int, d_q_ids_ptr: int, d_q_weights_ptr: int, k: int, d_ids_ptr: int, d_scores_ptr: int,
                               stream: int = 0, d_allow_ptr: int = 0, n_words: int = 0) -> None:
        r = self.lib.bert_hip_sparse_index_search_inverted_device(self.ix, n_queries, kq, d_q_ids_ptr, d_q_weights_ptr, k, d_allow_ptr or None,
                                                                  n_words, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._fail("bert_hip_sparse_index_search_inverted_device", r)

    def search_texts_inverted(self, texts: Sequence, kq: int = 32, k: int = 10, n_threads: int = 6):
        n = len(texts)
        txt = (C.c_char_p * n)(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        ids = np.empty((n, max(k, 1)), dtype=np.int32)
        scores = np.empty((n, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_sparse_index_search_inverted_texts(self.ix, n_threads, n, txt, kq, k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_sparse_index_search_inverted_texts", r)
        return ids, scores

    def get_rows(self, row_ids):
        """The stored rows: (ids [n, width] int32 ascending then -1, weights [n, width] float32, +0 behind the terms)."""
        row_ids = np.ascontiguousarray(row_ids, dtype=np.int32).reshape(-1)
        ids = np.empty((len(row_ids), self.width), dtype=np.int32)
        w = np.empty((len(row_ids), self.width), dtype=np.float32)
        r = self.lib.bert_hip_sparse_index_get_rows(self.ix, len(row_ids), row_ids.ctypes.data, ids.ctypes.data, w.ctypes.data)
        if r != 0:
            self._fail("bert_hip_sparse_index_get_rows", r)
        return ids, w


class BertTokenIndex:
    """bert_hip_token_index_*: documents' f16 token rows in HBM, exact MaxSim top-k search.  Documents and queries are (rows [n_tokens,
    dim] float32, cu [n + 1] int32) as BertModel.encode_tokens returns them.  search* / rescore* return (ids [n, k] int32, scores
    [n, k] f32), best first; missing entries are id -1, score -inf.  A ValueError is an argument the entry refused (-2).  The *_device
    forms take device pointers (ints) and a stream handle; search_device and rescore_device return at once."""

    DTYPES = {"f16": 1, "i8": 2}

    def __init__(self, model: BertModel, dim: Optional[int] = None, _load: Optional[str] = None, dtype: str = "f16"):
        self.model, self.lib = model, model.lib
        if dtype not in self.DTYPES:
            raise ValueError(f"dtype must be one of {sorted(self.DTYPES)}")
        self.dtype = dtype                                   # (a file holds f16 rows)
        if _load is not None:
            # dim comes from the file's header (include/bert_hip.h "LATE INDEX": u32 dim at byte 12)
            self.ix = self.lib.bert_hip_late_index_load(model.ctx, os.fsencode(_load))
            if not self.ix:
                raise RuntimeError("bert_hip_late_index_load failed (see stderr)")
            with open(_load, "rb") as f:
                self.dim = int(np.frombuffer(f.read(16), dtype="<u4")[3])
            return
        if dtype == "f16":
            self.ix = self.lib.bert_hip_token_index_create(model.ctx, 0 if dim is None else int(dim))
        else:
            self.ix = self.lib.bert_hip_late_index_create(model.ctx, 0 if dim is None else int(dim), self.DTYPES[dtype])
        if not self.ix:
            raise RuntimeError("bert_hip_token_index_create failed (see stderr)")
        self.dim = model.n_embd if dim is None else int(dim)

    def close(self):
        # (an index the context freed already — bert_free frees its indexes — must not be freed again)
        if getattr(self, "ix", None) and getattr(self.model, "ctx", None):
            self.lib.bert_hip_token_index_free(self.ix)
        self.ix = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return self.size()

    def size(self) -> int:
        return int(self.lib.bert_hip_token_index_size(self.ix))

    def n_tokens(self) -> int:
        return int(self.lib.bert_hip_token_index_n_tokens(self.ix))

    def max_query_tokens(self) -> int:
        return int(self.lib.bert_hip_token_index_max_query_tokens(self.ix))

    @staticmethod
    def _fail(name: str, r: int):
        if r == -2:
            raise ValueError(f"{name} refused its arguments (see stderr)")
        raise RuntimeError(f"{name} failed: {r}")

    def _packed(self, rows, cu):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        cu = np.ascontiguousarray(cu, dtype=np.int32).reshape(-1)
        if rows.ndim != 2 or rows.shape[1] != self.dim or len(cu) < 1:
            raise ValueError(f"rows must be [n_tokens, {self.dim}] and cu [n + 1]")
        if len(cu) > 1 and int(cu.max()) > len(rows):
            raise ValueError("cu names rows beyond the array")
        return rows, cu

    def reserve(self, n_docs: int, n_tokens: int, n_queries: int = 0, max_q_len: int = 0, k: int = 1) -> None:
        r = self.lib.bert_hip_token_index_reserve(self.ix, n_docs, n_tokens, n_queries, max_q_len, k)
        if r != 0:
            self._fail("bert_hip_token_index_reserve", r)

    def add(self, rows, cu) -> int:
        """documents (rows [n_tokens, dim] f32, cu [n_docs + 1]); returns the first new id."""
        rows, cu = self._packed(rows, cu)
        r = self.lib.bert_hip_token_index_add(self.ix, len(cu) - 1, cu.ctypes.data, rows.ctypes.data)
        if r < 0:
            self._fail("bert_hip_token_index_add", r)
        return r

    def add_device(self, cu, d_rows_ptr: int, stream: int = 0) -> int:
        """cu [n_docs + 1] on the HOST, d_rows_ptr f16 rows in device memory indexed by cu."""
        cu = np.ascontiguousarray(cu, dtype=np.int32).reshape(-1)
        r = self.lib.bert_hip_token_index_add_device(self.ix, len(cu) - 1, cu.ctypes.data, d_rows_ptr, stream)
        if r < 0:
            self._fail("bert_hip_token_index_add_device", r)
        return r

    def add_texts(self, texts: Sequence, n_threads: int = 6) -> int:
        n = len(texts)
        txt = (C.c_char_p * max(n, 1))(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        r = self.lib.bert_hip_token_index_add_texts(self.ix, n_threads, n, txt)
        if r < 0:
            self._fail("bert_hip_token_index_add_texts", r)
        return r

    def get_doc(self, doc_id: int) -> np.ndarray:
        """The stored rows of a document, [length, dim] float32 (the f16 values converted exactly)."""
        n = self.lib.bert_hip_token_index_get_doc(self.ix, doc_id, None, 0)
        if n < 0:
            self._fail("bert_hip_token_index_get_doc", n)
        rows = np.full((n, self.dim), np.nan, dtype=np.float32)
        if self.lib.bert_hip_token_index_get_doc(self.ix, doc_id, rows.ctypes.data, n) != n:
            raise RuntimeError("bert_hip_token_index_get_doc failed")
        return rows

    def get_codes(self, doc_id: int):
        """bert_hip_late_index_get_codes: the stored form of a document of an int8 index, (codes [length, dpad] int8, scales [length]
        f32); a ValueError on an f16 index."""
        n = self.lib.bert_hip_late_index_get_codes(self.ix, doc_id, None, None, 0)
        if n < 0:
            self._fail("bert_hip_late_index_get_codes", n)
        codes = np.full((n, (self.dim + 31) // 32 * 32), 99, dtype=np.int8)
        scales = np.full(n, np.nan, dtype=np.float32)
        if self.lib.bert_hip_late_index_get_codes(self.ix, doc_id, codes.ctypes.data, scales.ctypes.data, n) != n:
            raise RuntimeError("bert_hip_late_index_get_codes failed")
        return codes, scales

    def search(self, q_rows, q_cu, k: int = 10, allow=None):
        """allow: None, or the documents that may be returned — a bool array of len(index) entries or uint32 words (allow_words):
        bert_hip_late_index_search_filtered."""
        q, qcu = self._packed(q_rows, q_cu)
        nq = len(qcu) - 1
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        if allow is None:
            name = "bert_hip_token_index_search"
            r = self.lib.bert_hip_token_index_search(self.ix, nq, qcu.ctypes.data, q.ctypes.data, k, ids.ctypes.data, scores.ctypes.data)
        else:
            name = "bert_hip_late_index_search_filtered"
            words = allow_words(allow, len(self))
            r = self.lib.bert_hip_late_index_search_filtered(self.ix, nq, qcu.ctypes.data, q.ctypes.data, k, words.ctypes.data, len(words),
                                                             ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail(name, r)
        return ids, scores

    def search_device(self, n_queries: int, d_qcu_ptr: int, d_q_ptr: int, max_q_len: int, k: int, d_ids_ptr: int, d_scores_ptr: int,
                      stream: int = 0, d_allow_ptr: Optional[int] = None, n_words: int = 0) -> None:
        """d_allow_ptr: None (or 0), or device uint32 words [n_words] as search's allow (bert_hip_late_index_search_filtered_device)."""
        if d_allow_ptr:
            name = "bert_hip_late_index_search_filtered_device"
            r = self.lib.bert_hip_late_index_search_filtered_device(self.ix, n_queries, d_qcu_ptr, d_q_ptr, max_q_len, k, d_allow_ptr, n_words,
                                                                    d_ids_ptr, d_scores_ptr, stream)
        else:
            name = "bert_hip_token_index_search_device"
            r = self.lib.bert_hip_token_index_search_device(self.ix, n_queries, d_qcu_ptr, d_q_ptr, max_q_len, k, d_ids_ptr, d_scores_ptr, stream)
        if r != 0:
            self._fail(name, r)

    def search_texts(self, texts: Sequence, k: int = 10, n_threads: int = 6):
        n = len(texts)
        txt = (C.c_char_p * max(n, 1))(*[t if isinstance(t, bytes) else t.encode("utf-8") for t in texts])
        ids = np.empty((n, max(k, 1)), dtype=np.int32)
        scores = np.empty((n, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_token_index_search_texts(self.ix, n_threads, n, txt, k, ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_token_index_search_texts", r)
        return ids, scores

    def rescore(self, q_rows, q_cu, cand_ids, k: int = 10):
        """bert_hip_token_index_rescore: per query its candidate documents cand_ids [n, n_cand] (-1 = none) scored with the search's
        bits, the best k of them."""
        q, qcu = self._packed(q_rows, q_cu)
        nq = len(qcu) - 1
        cand = np.ascontiguousarray(cand_ids, dtype=np.int32).reshape(max(nq, 1), -1)
        ids = np.empty((nq, max(k, 1)), dtype=np.int32)
        scores = np.empty((nq, max(k, 1)), dtype=np.float32)
        r = self.lib.bert_hip_token_index_rescore(self.ix, nq, qcu.ctypes.data, q.ctypes.data, cand.shape[1], cand.ctypes.data, k,
                                                  ids.ctypes.data, scores.ctypes.data)
        if r != 0:
            self._fail("bert_hip_token_index_rescore", r)
        return ids, scores

    def rescore_device(self, n_queries: int, d_qcu_ptr: int, d_q_ptr: int, n_cand: int, d_cand_ptr: int, k: int, d_ids_ptr: int,
                       d_scores_ptr: int, stream: int = 0) -> None:
        r = self.lib.bert_hip_token_index_rescore_device(self.ix, n_queries, d_qcu_ptr, d_q_ptr, n_cand, d_cand_ptr, k, d_ids_ptr, d_scores_ptr,
                                                         stream)
        if r != 0:
            self._fail("bert_hip_token_index_rescore_device", r)

    def remove(self, ids) -> int:
        """bert_hip_late_index_remove: the number of documents newly removed."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        r = self.lib.bert_hip_late_index_remove(self.ix, len(ids), ids.ctypes.data)
        if r < 0:
            self._fail("bert_hip_late_index_remove", r)
        return r

    def n_live(self) -> int:
        return int(self.lib.bert_hip_late_index_n_live(self.ix))

    def n_live_tokens(self) -> int:
        return int(self.lib.bert_hip_late_index_n_live_tokens(self.ix))

    def compact(self) -> np.ndarray:
        """bert_hip_late_index_compact: drops the removed documents; returns the former ids of the documents now at 0 .. len(index) - 1."""
        old = np.empty(max(self.n_live(), 1), dtype=np.int32)
        r = self.lib.bert_hip_late_index_compact(self.ix, old.ctypes.data)
        if r < 0:
            self._fail("bert_hip_late_index_compact", r)
        return old[:r]

    def save(self, path: str) -> None:
        r = self.lib.bert_hip_late_index_save(self.ix, os.fsencode(path))
        if r != 0:
            self._fail("bert_hip_late_index_save", r)

    def live_ids(self) -> np.ndarray:
        """The ids a search can return, ascending.  With removed documents: found by rescoring every id against a one-token query, 256
        candidates per query (a removed document is skipped; a document whose score is NaN is not found either)."""
        n = len(self)
        if self.n_live() == n:
            return np.arange(n, dtype=np.int32)
        cand = np.full((n + 255) // 256 * 256, -1, np.int32)
        cand[:n] = np.arange(n, dtype=np.int32)
        nq = len(cand) // 256
        ids, _ = self.rescore(np.zeros((nq, self.dim), np.float32), np.arange(nq + 1, dtype=np.int32), cand.reshape(-1, 256), 256)
        return np.sort(ids[ids >= 0])


def test_gemm(A: np.ndarray, W_bytes: np.ndarray, wtype: int, N: int, bias: np.ndarray,
              resid: Optional[np.ndarray], epilogue: int, impl: int) -> np.ndarray:
    """A: float16 [M, K]; W_bytes: file-layout bytes of W[N][K]; returns float16 [M, N]."""
    L = test_lib()
    A = np.ascontiguousarray(A, dtype=np.float16)
    M, K = A.shape
    Wb = np.ascontiguousarray(W_bytes)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    out = np.zeros((M, N), dtype=np.float16)
    rp = None
    if resid is not None:
        resid = np.ascontiguousarray(resid, dtype=np.float16)
        rp = resid.ctypes.data
    r = L.bert_hip_test_gemm(M, N, K, A.ctypes.data, Wb.ctypes.data, wtype, bias.ctypes.data, rp, epilogue, impl,
                             out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_gemm failed: {r}")
    return out


def test_gemm_lnfold(A1, W1, b1, r, rg, rb, W2, b2, g, be, epi2):
    """The LayerNorm-folded mat-mul pair of the H = 768 route (include/bert_hip_test.h): returns (u [M,H] f16, out2 [M,N2] f16, rows [M,4] f32)."""
    L = test_lib()
    A1 = np.ascontiguousarray(A1, dtype=np.float16); W1 = np.ascontiguousarray(W1, dtype=np.float16); W2 = np.ascontiguousarray(W2, dtype=np.float16)
    r = np.ascontiguousarray(r, dtype=np.float16)
    f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float32)
    b1, rg, rb, b2, g, be = f(b1), f(rg), f(rb), f(b2), f(g), f(be)
    M, K1 = A1.shape
    H, N2 = W1.shape[0], W2.shape[0]
    u = np.zeros((M, H), dtype=np.float16); out = np.zeros((M, N2), dtype=np.float16); rows = np.zeros((M, 4), dtype=np.float32)
    p = lambda v: None if v is None else v.ctypes.data
    rc = L.bert_hip_test_gemm_lnfold(M, K1, H, N2, p(A1), p(W1), p(b1), p(r), p(rg), p(rb), p(W2), p(b2), p(g), p(be), epi2, p(u), p(out), p(rows))
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_gemm_lnfold failed: {rc}")
    return u, out, rows


def test_attention(qkv: np.ndarray, cu_seqlens: np.ndarray, n_head: int, d_head: int, impl: int) -> np.ndarray:
    L = test_lib()
    qkv = np.ascontiguousarray(qkv, dtype=np.float16)
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    T = qkv.shape[0]
    out = np.zeros((T, n_head * d_head), dtype=np.float16)
    r = L.bert_hip_test_attention(len(cu) - 1, _i32p(cu), n_head, d_head, qkv.ctypes.data, impl, out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_attention failed: {r}")
    return out


def test_attention_bias(qkv: np.ndarray, cu_seqlens: np.ndarray, n_head: int, d_head: int, impl: int, W: Optional[np.ndarray], P: int,
                        rel: Optional[np.ndarray] = None) -> np.ndarray:
    """test_attention with MPNet's relative position bias W [32][n_head] f32, expanded for sentences of up to P tokens; rel, if given,
    is a table [n_head][2 P - 1] f32 taken as it is in place of the expansion (impl 0 wants it times sqrt(d_head))."""
    L = test_lib()
    qkv = np.ascontiguousarray(qkv, dtype=np.float16)
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros((qkv.shape[0], n_head * d_head), dtype=np.float16)
    if W is not None:
        W = np.ascontiguousarray(W, dtype=np.float32)
        assert W.shape == (32, n_head)
    if rel is not None:
        rel = np.ascontiguousarray(rel, dtype=np.float32)
        assert rel.shape == (n_head, 2 * P - 1)
    r = L.bert_hip_test_attention_bias(len(cu) - 1, _i32p(cu), n_head, d_head, qkv.ctypes.data, impl, out.ctypes.data,
                                       W.ctypes.data if W is not None else None, P, rel.ctypes.data if rel is not None else None)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_attention_bias failed: {r}")
    return out


def test_rel_bias_table(W: np.ndarray, P: int) -> np.ndarray:
    """The host expansion of W [32][n_head] f32: rel [n_head][2 P - 1], rel[h][d + P - 1] = W[bucket(d)][h] (no device)."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    assert W.ndim == 2 and W.shape[0] == 32
    out = np.zeros((W.shape[1], 2 * P - 1), dtype=np.float32)
    r = test_lib().bert_hip_test_rel_bias_table(W.ctypes.data, W.shape[1], P, out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_rel_bias_table failed: {r}")
    return out


def test_qkv_attention(x: np.ndarray, cu_seqlens: np.ndarray, n_head: int, d_head: int, W_bytes: np.ndarray, wtype: int,
                       bias: np.ndarray, fused: bool) -> np.ndarray:
    """x [T][H] f16, Wqkv [3H][H] in file layout of wtype, bias [3H] -> attention context [T][H] f16."""
    L = test_lib()
    x = np.ascontiguousarray(x, dtype=np.float16)
    cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    w = np.ascontiguousarray(W_bytes)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    out = np.zeros((x.shape[0], n_head * d_head), dtype=np.float16)
    r = L.bert_hip_test_qkv_attention(len(cu) - 1, _i32p(cu), n_head, d_head, x.ctypes.data, w.ctypes.data, wtype,
                                      bias.ctypes.data, int(fused), out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_qkv_attention failed: {r}")
    return out


def test_layer_tail(ctx: np.ndarray, x: np.ndarray, Wo_bytes, W1_bytes, W2_bytes, wtype: int, I: int, bo, g1, be1, b1, b2,
                    g2, be2, impl: int) -> np.ndarray:
    """ctx, x [M][H] f16 -> layer output [M][H] f16 (out-projection + LN + FFN + LN); impl see bert_hip.h."""
    L = test_lib()
    ctx = np.ascontiguousarray(ctx, dtype=np.float16)
    x = np.ascontiguousarray(x, dtype=np.float16)
    M, H = ctx.shape
    ws = [np.ascontiguousarray(w) for w in (Wo_bytes, W1_bytes, W2_bytes)]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    ps = [f(v) for v in (bo, g1, be1, b1, b2, g2, be2)]
    out = np.zeros((M, H), dtype=np.float16)
    r = L.bert_hip_test_layer_tail(M, H, I, ctx.ctypes.data, x.ctypes.data, ws[0].ctypes.data, ws[1].ctypes.data,
                                   ws[2].ctypes.data, wtype, *[p.ctypes.data for p in ps], impl, out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_layer_tail failed: {r}")
    return out


def test_skinny_tail(ctx: np.ndarray, x: np.ndarray, Wo_bytes, W1_bytes, W2_bytes, wtype: int, I: int, bo, g1, be1, b1, b2,
                     g2, be2, pad: int = 0, parts: bool = False):
    """test_layer_tail's operation through the latency route's kernels; pad: the 16-bit pattern in the padding rows of ctx and x.
    parts: returns (out, {"v_proj" f32 [M][H], "y" f16 [M][H], "ff" f16 [M][I] in fragment order, "v_down" f32 [M][H]})."""
    L = test_lib()
    ctx = np.ascontiguousarray(ctx, dtype=np.float16)
    x = np.ascontiguousarray(x, dtype=np.float16)
    M, H = ctx.shape
    ws = [np.ascontiguousarray(w) for w in (Wo_bytes, W1_bytes, W2_bytes)]
    ps = [np.ascontiguousarray(v, dtype=np.float32) for v in (bo, g1, be1, b1, b2, g2, be2)]
    out = np.zeros((M, H), dtype=np.float16)
    mid = {"v_proj": np.zeros((M, H), dtype=np.float32), "y": np.zeros((M, H), dtype=np.float16),
           "ff": np.zeros((M, I), dtype=np.float16), "v_down": np.zeros((M, H), dtype=np.float32)} if parts else {}
    r = L.bert_hip_test_skinny_tail(M, H, I, ctx.ctypes.data, x.ctypes.data, ws[0].ctypes.data, ws[1].ctypes.data, ws[2].ctypes.data,
                                    wtype, *[p.ctypes.data for p in ps], pad, out.ctypes.data,
                                    *[mid[k].ctypes.data if parts else None for k in ("v_proj", "y", "ff", "v_down")])
    if r != 0:
        raise RuntimeError(f"bert_hip_test_skinny_tail failed: {r}")
    return (out, mid) if parts else out


def test_skinny_qkv(W_bytes: np.ndarray, wtype: int, bias: np.ndarray, x: Optional[np.ndarray] = None, V: Optional[np.ndarray] = None,
                    gamma=None, beta=None, pad: int = 0):
    """The latency route's Q|K|V projection of x [M][H] f16 -> qkv [M][3H] f16, or of LayerNorm(V [M][H] f32; gamma, beta), which the
    kernel computes itself -> (qkv, the normalised rows [M][H] f16).  pad: the 16-bit (x) / 32-bit (V) pattern of the padding rows."""
    L = test_lib()
    w = np.ascontiguousarray(W_bytes)
    bias = np.ascontiguousarray(bias, dtype=np.float32)
    rows = np.ascontiguousarray(x, dtype=np.float16) if V is None else np.ascontiguousarray(V, dtype=np.float32)
    M, H = rows.shape
    qkv = np.zeros((M, 3 * H), dtype=np.float16)
    if V is None:
        r = L.bert_hip_test_skinny_qkv(M, H, rows.ctypes.data, None, None, None, w.ctypes.data, wtype, bias.ctypes.data, pad, qkv.ctypes.data, None)
    else:
        g = np.ascontiguousarray(gamma, dtype=np.float32); b = np.ascontiguousarray(beta, dtype=np.float32)
        ln_out = np.zeros((M, H), dtype=np.float16)
        r = L.bert_hip_test_skinny_qkv(M, H, None, rows.ctypes.data, g.ctypes.data, b.ctypes.data, w.ctypes.data, wtype, bias.ctypes.data, pad,
                                       qkv.ctypes.data, ln_out.ctypes.data)
    if r != 0:
        raise RuntimeError(f"bert_hip_test_skinny_qkv failed: {r}")
    return qkv if V is None else (qkv, ln_out)


# ---- the f32 route's kernels (include/bert_hip_test.h bert_hip_test_f32_*): f32 arrays in, f32 arrays out ----
def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def test_f32_gemm(A: np.ndarray, W: np.ndarray, bias: np.ndarray, resid: Optional[np.ndarray], epilogue: int) -> np.ndarray:
    """epilogue(A [M,K] W [N,K]^T + bias): 0 bias, 1 bias + GELU, 2 bias + resid [M,N]."""
    A, W, bias = _f32c(A), _f32c(W), _f32c(bias)
    (M, K), N = A.shape, W.shape[0]
    assert W.shape == (N, K) and bias.shape == (N,)
    r = None if resid is None else _f32c(resid)
    assert r is None or r.shape == (M, N)
    C_ = np.zeros((M, N), dtype=np.float32)
    rc = test_lib().bert_hip_test_f32_gemm(M, N, K, A.ctypes.data, W.ctypes.data, bias.ctypes.data, None if r is None else r.ctypes.data,
                                           epilogue, C_.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_gemm failed: {rc}")
    return C_


def test_f32_attention(qkv: np.ndarray, cu_seqlens, n_head: int, d_head: int, max_len: int) -> np.ndarray:
    qkv = _f32c(qkv); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    assert qkv.shape == (int(cu[-1]), 3 * n_head * d_head)
    out = np.zeros((qkv.shape[0], n_head * d_head), dtype=np.float32)
    rc = test_lib().bert_hip_test_f32_attention(len(cu) - 1, _i32p(cu), n_head, d_head, max_len, qkv.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_attention failed: {rc}")
    return out


def test_f32_attention_bias(qkv: np.ndarray, cu_seqlens, n_head: int, d_head: int, max_len: int, W: np.ndarray, P: int) -> np.ndarray:
    """test_f32_attention with MPNet's relative position bias W [32][n_head] f32, expanded for sentences of up to P tokens."""
    qkv = _f32c(qkv); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32); W = _f32c(W)
    assert qkv.shape == (int(cu[-1]), 3 * n_head * d_head) and W.shape == (32, n_head)
    out = np.zeros((qkv.shape[0], n_head * d_head), dtype=np.float32)
    rc = test_lib().bert_hip_test_f32_attention_bias(len(cu) - 1, _i32p(cu), n_head, d_head, max_len, qkv.ctypes.data, out.ctypes.data, W.ctypes.data, P)
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_attention_bias failed: {rc}")
    return out


def test_f32_layernorm(x: np.ndarray, gamma, beta) -> np.ndarray:
    x, g, b = _f32c(x), _f32c(gamma), _f32c(beta)
    out = np.zeros_like(x)
    rc = test_lib().bert_hip_test_f32_layernorm(x.shape[0], x.shape[1], x.ctypes.data, g.ctypes.data, b.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_layernorm failed: {rc}")
    return out


def test_f32_embed_ln(word, type_, pos, gamma, beta, tokens, cu_seqlens, max_len: int) -> np.ndarray:
    word, type_, pos, g, b = (_f32c(a) for a in (word, type_, pos, gamma, beta))
    toks = np.ascontiguousarray(tokens, dtype=np.int32); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    H = word.shape[1]
    assert type_.shape == (2, H) and pos.shape[1] == H and len(toks) == int(cu[-1])
    out = np.zeros((len(toks), H), dtype=np.float32)
    rc = test_lib().bert_hip_test_f32_embed_ln(H, word.shape[0], pos.shape[0], word.ctypes.data, type_.ctypes.data, pos.ctypes.data,
                                               g.ctypes.data, b.ctypes.data, _i32p(toks), _i32p(cu), len(cu) - 1, max_len, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_embed_ln failed: {rc}")
    return out


def test_f32_pool(x: np.ndarray, cu_seqlens, max_len: int, pooling: str = "mean", normalize: bool = True):
    """test_pool on f32 rows: (rows [n_sentences, H] f32, status word)."""
    x = _f32c(x); cu = np.ascontiguousarray(cu_seqlens, dtype=np.int32)
    out = np.zeros((len(cu) - 1, x.shape[1]), dtype=np.float32)
    st = np.zeros(1, dtype=np.int32)
    rc = test_lib().bert_hip_test_f32_pool(x.shape[1], x.ctypes.data, _i32p(cu), len(cu) - 1, max_len, {"mean": 0, "cls": 1}[pooling],
                                           int(bool(normalize)), out.ctypes.data, _i32p(st))
    if rc != 0:
        raise RuntimeError(f"bert_hip_test_f32_pool failed: {rc}")
    return out, int(st[0])
