// options.cpp — see options.h.  The one translation unit that is compiled twice: libbert_test.so's copy (-DBERT_HIP_TEST_ROUTES)
// also understands the whole-model "naive" route and the "test_poison_*" keys.
#include "options.h"

#include <cstdio>
#include <cstdlib>

#include "weights.h"

namespace bert_hip {

// The GENERIC kernels (any shape, row-major f16 images) are what shapes outside the MFMA kernels' reach fall back to; running a
// whole model on them is a cross-check for the tests, not a route of the product.
#ifdef BERT_HIP_TEST_ROUTES
static constexpr bool TEST_ROUTES = true;
#else
static constexpr bool TEST_ROUTES = false;
#endif

int EngineOptions::pool_mode() const { return (pool_cls ? POOL_CLS : 0) | (normalize ? 0 : POOL_RAW); }

// A key and its value, with no questions asked (but of the two that change what a context computes: they take the values they
// name and nothing else): the parsing the environment and bert_hip_set_option share.
void EngineOptions::apply(const std::string &key, const std::string &value) {
    const int n = atoi(value.c_str());
    if (key == "pooling" || key == "normalize") {
        const bool pooling = key == "pooling";
        const char *const on = pooling ? "cls" : "1", *const off = pooling ? "mean" : "0";
        if (value == on || value == off) (pooling ? pool_cls : normalize) = value == on;
        else fprintf(stderr, "bert_hip: %s = \"%s\": expected \"%s\" or \"%s\"; ignored\n", key.c_str(), value.c_str(), off, on);
        return;
    }
    if (key == "gemm") gemm_naive = value == "naive";
    else if (key == "attn") attn_naive = value == "naive";
    else if (key == "qkv2") qkv2 = value != "0";
    else if (key == "gemm256") gemm256 = value != "0";
    else if (key == "ln_fold") ln_fold = value != "0";
    else if (key == "tail") tail = value != "0";
    else if (key == "latency") latency = value != "0";
    else if (key == "stage_kernel") stage_kernel = value != "0";
    else if (key == "window_slots") set_window_slots(n);      // (process-wide, not this engine's: 16, or 8 — see kernels.h)
    else if (key == "latency_tokens") { if (n >= 32) latency_tokens = n; }
    else if (key == "one_launch") one_launch = value == "0" ? 0 : value == "2" ? 2 : 1;
    else if (key == "f32") f32_exact = value != "f16";        // f32 files: "exact" (f32 arithmetic, default) | "f16" (f16 operands, fused kernels)
    else if (key == "chunk_tokens") { if (n > 0) chunk_tokens = n; }
    else if (key == "sparse_index_qb") sparse_index_qb = n >= 1 && n <= 8 ? n : 0;
    else if (key == "sparse_index_segment_rows") sparse_index_segment_rows = n >= 256 && n <= 16384 && n % 256 == 0 ? n : 0;
    else if (key == "hybrid_chunk_queries") hybrid_chunk_queries = n >= 1 && n <= 4096 ? n : 0;
    else if (key == "token_index_slices") token_index_slices = n >= 1 && n <= 4096 ? n : 0;
    else if (key == "maxsim_launch_pairs") maxsim_launch_pairs = n >= 1 ? (n < MAXSIM_LAUNCH_PAIRS ? n : MAXSIM_LAUNCH_PAIRS) : 0;
}

// Where the environment differs from the keys:
//   BERT_HIP_KERNELS  no key: "tiled" clears four switches together, "naive" sets "gemm" and "attn" BEFORE the weights are
//                     packed, which is what builds the generic kernels' images ("gemm" = "naive" alone cannot, later)
//   BERT_HIP_LATENCY  the keys "latency" and "latency_tokens" in one: 0 = no latency route; 1 = the default cap; n >= 32: calls of
//                     at most n tokens take it
//   BERT_HIP_Q4       no key: decides how the weights are packed
// "qkv2", "gemm256", "tail", "stage_kernel", "one_launch", "sparse_index_qb", "sparse_index_segment_rows", "hybrid_chunk_queries", "token_index_slices", "maxsim_launch_pairs" (and the profiler's "profile_replay") are keys only.
EngineOptions EngineOptions::from_env(const HParams &hp) {
    EngineOptions o;
    // (the cap of the latency route: measured on H = 384; a window of an H = 128 model costs the fused kernels less than five
    // launches cost the route, so such models keep the one-window cap)
    if (hp.n_embd < 256) o.latency_tokens = 128;
    // BERT_HIP_KERNELS = fused (default) | tiled (GEMM + attention + LayerNorm kernels, Q|K|V and the intermediate through HBM)
    const std::string kernels = getenv("BERT_HIP_KERNELS") ? getenv("BERT_HIP_KERNELS") : "";
    if (kernels == "naive" && TEST_ROUTES) o.gemm_naive = o.attn_naive = true;
    else if (kernels == "naive") fprintf(stderr, "BERT_HIP_KERNELS=naive: a test cross-check (libbert_test.so), not a route of libbert.so; ignored\n");
    else if (kernels == "tiled") o.qkv2 = o.tail = o.latency = false, o.one_launch = 0;
    if (const char *v = getenv("BERT_HIP_Q4")) o.q4_expand = std::string(v) != "fused";
    static const char *const same_as_key[][2] = {
        {"BERT_HIP_LATENCY", "latency"}, {"BERT_HIP_LATENCY", "latency_tokens"},
        {"BERT_HIP_LN_FOLD", "ln_fold"},                      // (tuning: 0 = LayerNorm kernels of their own at H = 768)
        {"BERT_HIP_CHUNK_TOKENS", "chunk_tokens"}, {"BERT_HIP_WINDOW_SLOTS", "window_slots"},
        {"BERT_HIP_F32", "f32"},                              // (f32 files: f32 arithmetic like the reference's unless "f16")
        {"BERT_HIP_POOLING", "pooling"}, {"BERT_HIP_NORMALIZE", "normalize"},
    };
    for (auto &ek : same_as_key)
        if (const char *v = getenv(ek[0])) o.apply(ek[1], v);
    return o;
}

void EngineOptions::set(const std::string &key, const std::string &value, bool naive_images, bool fold_images) {
    if (!TEST_ROUTES && (key == "gemm" || key == "attn") && value == "naive")
        fprintf(stderr, "bert_hip_set_option: %s=naive is a test cross-check (libbert_test.so), not a route of libbert.so; ignored\n", key.c_str());
    // the generic kernel reads GemmWeight::naive16, an image that is only built at load time (BERT_HIP_KERNELS=naive) or
    // for shapes the MFMA kernels cannot take: refuse the switch when a matrix lacks it
    else if (key == "gemm" && value == "naive" && !naive_images)
        fprintf(stderr, "bert_hip_set_option: gemm=naive needs BERT_HIP_KERNELS=naive at load time (the f16 row-major images were not built); ignored\n");
    else if (key == "ln_fold" && value != "0" && !fold_images)
        fprintf(stderr, "bert_hip_set_option: ln_fold=1 needs BERT_HIP_LN_FOLD=1 at load time (the folded images were not built); ignored\n");
    else apply(key, value);
}

bool test_poison_option(const std::string &key, const DevBuf &ctx, const DevBuf &xres, std::initializer_list<const DevBuf *> workspace) {
    if (!TEST_ROUTES || (key != "test_poison_ctx" && key != "test_poison_xres" && key != "test_poison_workspace")) return false;
    auto poison = [](const DevBuf &buf) { if (buf.p) (void)hipMemset(buf.p, 0xFF, buf.bytes); };
    (void)hipDeviceSynchronize();
    if (key == "test_poison_workspace") for (const DevBuf *buf : workspace) poison(*buf);
    else poison(key == "test_poison_ctx" ? ctx : xres);
    (void)hipDeviceSynchronize();
    return true;
}

}  // namespace bert_hip
