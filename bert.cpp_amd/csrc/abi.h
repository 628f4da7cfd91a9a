// abi.h — what the files that hold extern "C" entry points (bert_api.cpp, index_api.cpp) share.
#pragma once
#include <cstdint>
#include <cstdio>
#include <exception>
#include <type_traits>
#include <utility>

#include "context.h"

namespace bert_hip {

// No exception may cross the C ABI: every extern "C" entry runs its body through this; an exception
// (std::bad_alloc from a staging vector, std::system_error from a thread, ...) becomes the reference's error convention — a
// line on stderr and an early return (of on_error, unless the entry returns nothing) with the outputs untouched.
struct no_result {};
template <class F, class R = no_result>
auto guarded(const char *name, F &&body, R on_error = {}) -> decltype(body()) {
    try {
        return body();
    } catch (const std::exception &e) {
        fprintf(stderr, "%s: %s\n", name, e.what());
    } catch (...) {
        fprintf(stderr, "%s: unknown exception\n", name);
    }
    if constexpr (!std::is_void_v<decltype(body())>) return on_error;
}

// closes the file a load entry point opened, on every way out
struct FileCloser {
    void operator()(FILE *f) const { if (f) fclose(f); }
};

// bert_encode_batch / bert_hip_encode_batch: number of inputs encoded (stops at the first failure, later outputs untouched), -1
// for a context without a device
int32_t encode_batch_impl(bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, float **embeddings);

// bert_hip_encode_long_batch: number of inputs encoded, -1 for a context without a device, -2 (outputs untouched) for a bad window or stride
int32_t encode_long_batch_impl(bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window, int32_t stride,
                               float **embeddings, int32_t *n_windows);
bool long_args_ok(const char *me, const bert_ctx *ctx, int32_t window, int32_t stride);

}  // namespace bert_hip
