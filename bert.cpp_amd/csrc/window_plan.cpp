// window_plan.cpp — see window_plan.h.
#include "window_plan.h"

namespace bert_hip {

int32_t plan_windows(int32_t n_tokens, int32_t window, int32_t stride, int32_t *starts, int32_t cap) {
    if (n_tokens < 2 || window < 3 || stride < 1 || stride > window - 2) return -2;
    if (n_tokens <= window) {
        if (cap >= 1 && starts) starts[0] = 0;
        return 1;
    }
    const int64_t m = (int64_t)n_tokens - 2, c = (int64_t)window - 2;
    const int64_t count = 1 + (m - c + stride - 1) / stride;
    if (count > INT32_MAX) return -2;
    if (cap >= count && starts) {
        int32_t i = 0;
        for (int64_t s = 0; s + c < m; s += stride) starts[i++] = (int32_t)s;
        starts[i] = (int32_t)(m - c);
    }
    return (int32_t)count;
}

}  // namespace bert_hip
