// window_plan.h — how a text longer than a window is cut into overlapping windows (bert_hip.h "long texts": bert_hip_plan_windows,
// bert_hip_encode_long_batch).  No device code: the text entry points build their sentences from what this returns, and a test
// reaches it without a device.
#pragma once
#include <cstdint>

namespace bert_hip {

// The windows of a text of n_tokens ids ([CLS] ... [SEP]).  window counts all ids of a window, its [CLS] and [SEP] included, stride
// counts inner ids; m = n_tokens - 2 inner ids, c = window - 2.  n_tokens <= window: one window, the text itself (start 0).  Else
// windows of exactly c inner ids start at 0, stride, 2 stride, ... while start + c < m, and one last window starts at m - c:
// 1 + ceil((m - c) / stride) windows, the first at the text's start, the last at its end, every inner id in at least one.
// Returns the number of windows, and writes starts[0 .. count) if cap >= count (nothing otherwise; starts may be null then);
// -2 unless n_tokens >= 2, window >= 3 and 1 <= stride <= window - 2.
int32_t plan_windows(int32_t n_tokens, int32_t window, int32_t stride, int32_t *starts, int32_t cap);

}  // namespace bert_hip
