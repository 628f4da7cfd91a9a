// text_batch.h — the host side of the text entry points (bert_encode_batch, bert_hip_tokenize_batch, the index's *_texts):
// texts are tokenized on a pool of host threads, validated and packed into the form the engine takes (ids back to back +
// prefix sums), group by group, the next group on a thread of its own while the caller evaluates the current one.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "multi_device.h"
#include "tokenizer.h"
#include "window_plan.h"

namespace bert_hip {

struct TextBatcher;

// A group of tokenized texts.  Buffers are kept between calls, grown only and never zero-filled (the tokenizer writes what is
// read; 16384 texts x n_max_tokens ids are 32 MiB of pages to touch otherwise).
struct TokenGroup {
    std::unique_ptr<int32_t[]> ids, packed;            // [n][n_max_tokens] as tokenized; the same ids back to back
    size_t ids_cap = 0, packed_cap = 0;
    std::vector<int32_t> n_tokens, cu;                  // [n] counts; [n_ok + 1] prefix sums
    int32_t n_ok = 0;                                   // texts in front of the first one the engine cannot take (= all of them)

    // tokenizes n texts on the batcher's threads and packs them
    void tokenize(TextBatcher &tb, int32_t n_threads, int32_t n, const char **texts);
    // n_tokens[0..n) and ids -> cu, n_ok, packed.  A text can be evaluated if its count is 1 .. n_max_tokens (the tokenizer's
    // ids are in range by construction; its counts are 2 .. n_max_tokens)
    void pack(int32_t n_max_tokens, int32_t n);
};

// texts of group k (0, 1, ...) of a call with `left` texts to go: the groups GROW — 2048, 4096, 8192, then 16384 texts: the first
// one is all a caller waits for with an idle GPU, later ones amortise the fixed costs of a blocking evaluation and fill the GPU
// better (1.17 M texts/s at 2048 texts of 25 tokens, 1.37 M at 16384); a remainder of less than a quarter of a group joins the
// last one.  Tokenizing a group of twice the size still fits under its predecessor's evaluation.
int32_t encode_group_size(int k, int32_t left);

// A group of LONG texts as the engine takes it (bert_hip.h "long texts"): every window of every text an ordinary sentence, one group
// of consecutive sentences per text.
struct LongGroup {
    std::vector<int32_t> packed, cu, group_cu;          // the windows' ids back to back; [n_windows + 1]; [n_texts + 1]
    int32_t n_texts() const { return (int32_t)group_cu.size() - 1; }
    int32_t n_windows() const { return (int32_t)cu.size() - 1; }
    void clear() { packed.clear(); cu.assign(1, 0); group_cu.assign(1, 0); }
    // the windows of one text (ids: all of them, [CLS] ... [SEP]; window, stride: legal for plan_windows) as sentences of a new group:
    // window i is ids[0], the window's inner ids from 1 + starts[i], ids[last].  Returns their number.
    int32_t append(const std::vector<int32_t> &ids, int32_t window, int32_t stride);
};
// windows a group of long texts holds at most (a text's windows never straddle two groups; a text with more is a group of its own)
constexpr int32_t LONG_GROUP_WINDOWS = 16384;

// The text pipeline of a context.  Not re-entrant, like every entry point of a bert_ctx (context.h).
struct TextBatcher {
    const Tokenizer *tok = nullptr;                     // the context's, set at load
    int32_t n_max_tokens = 0;
    // host threads of the batch tokenizer, created at the first call that asks for them and kept: a group of 4096 texts
    // tokenizes in about a millisecond, sixteen thread starts cost a third of that
    std::unique_ptr<ShardWorkers> workers;
    int workers_asked = 0;
    // two groups of tokenized texts: one on the GPU, one being tokenized
    TokenGroup group[2];

    // Tokenizes n_inputs texts into tokens[i * n_max_tokens ..] on up to n_threads host threads (the tokenizer itself is const
    // and re-entrant; inputs are handed out in blocks of 16 from a shared counter).
    void tokenize_many(int32_t n_threads, int32_t n_inputs, const char **texts, int32_t *tokens, int32_t *n_tokens);

    // Inputs go through in groups (encode_group_size): group g+1 is tokenized AND PACKED while eval(group g, first text of g)
    // runs (cu_seqlens and the ids back to back, what bert_eval_batch would do first thing with the GPU idle: 0.1 us per text,
    // 1.7 ms for 16384), and the id buffers stay bounded for any n_inputs.  eval evaluates the group's n_ok texts and returns
    // their number, or -1.  Returns the number of inputs encoded: stops at the first text that cannot be evaluated (a line on
    // stderr) or the first failed eval, later outputs untouched.
    using EvalGroup = std::function<int32_t(const TokenGroup &g, int32_t i0)>;
    int32_t encode_groups(int32_t n_threads, int32_t n_inputs, const char **texts, const EvalGroup &eval);

    // All ids of a text, [CLS] ... [SEP], without truncation: the buffer is sized from the text's byte length (a text of b bytes
    // yields at most b + 2 ids — every id consumes a byte —, so Tokenizer::tokenize with that cap never truncates).
    void tokenize_long(const char *text, std::vector<int32_t> &ids) const;
    // Long texts (bert_hip.h): tokenized without truncation on up to n_threads host threads, a slab of texts at a time, cut into
    // windows (plan_windows; window and stride validated by the caller) and handed to eval in groups of at most LONG_GROUP_WINDOWS
    // windows.  eval evaluates the group (texts i0 .. i0 + n_texts - 1) and returns n_texts, or -1.  Tokenizing and evaluating take
    // turns (no group is tokenized under its predecessor's evaluation).  n_windows (nullable): [n_inputs], written per evaluated
    // group.  Returns the number of inputs encoded: stops at the first failed eval, later outputs untouched.
    using EvalLongGroup = std::function<int32_t(const LongGroup &g, int32_t i0)>;
    int32_t encode_long_groups(int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window, int32_t stride, int32_t *n_windows,
                               const EvalLongGroup &eval);
    LongGroup long_group;
};

}  // namespace bert_hip
