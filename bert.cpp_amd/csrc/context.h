// context.h — struct bert_ctx: what a loaded model owns (tokenizer, one engine per GPU, the host threads and buffers of the
// batch entry points, the embedding gather, the caller's indexes, sparse indexes and token indexes), and how it is loaded.
//
// A context is NOT thread-safe, like the reference's: every entry point that takes one may use its worker pools and its
// grow-only buffers, so calls on one context are serialised by the caller (bert_encode_batch's tokenize-ahead thread is the
// only second thread a context ever sees, and the call that started it waits for it).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "gather.h"
#include "multi_device.h"
#include "search.h"
#include "sparse_index.h"
#include "text_batch.h"
#include "token_index.h"
#include "tokenizer.h"

struct bert_ctx;

// an embedding index (search.h) and the context it was made from
struct bert_hip_index {
    bert_ctx *ctx = nullptr;
    std::unique_ptr<bert_hip::Index> ix;
};

// a sparse index (sparse_index.h) and the context it was made from
struct bert_hip_sparse_index {
    bert_ctx *ctx = nullptr;
    std::unique_ptr<bert_hip::SparseIndex> ix;
};

// a token index (token_index.h) and the context it was made from
struct bert_hip_token_index {
    bert_ctx *ctx = nullptr;
    std::unique_ptr<bert_hip::TokenIndex> ix;
};

struct bert_ctx {
    bert_hip::HParams hp;
    // the model file holds MPNet's relative position bias (model_file.h): tok wraps a text in <s> ... </s>, the pair routes refuse
    bool rel_bias = false;
    bert_hip::Tokenizer tok;
    // one engine (weight replica + stream + workspace) per GPU; empty for tokenizer-only contexts.  Devices:
    // BERT_HIP_DEVICES ("all" or a comma-separated list without repeats), else the
    // calling thread's CURRENT device — one context = one GPU unless the caller asks for more, like the reference's one
    // context = one compute arena (eight torch.distributed ranks that each load a model must not build 64 replicas)
    std::vector<std::unique_ptr<bert_hip::Engine>> engines;
    // host threads of the devices beyond the first, created once at load (multi_device.h)
    std::unique_ptr<bert_hip::ShardWorkers> workers;
    // the batch tokenizer's threads and the two groups of tokenized texts of the text entry points (text_batch.h)
    bert_hip::TextBatcher texts;
    // test knob (bert_hip_set_option "test_inject_bad_alloc"): the ABI's catch-all
    bool inject_bad_alloc = false;
    // device-resident results of bert_hip_eval_packed_gather; declared behind the engines: its streams are drained and its
    // buffers freed before the engines go
    bert_hip::EmbeddingGather gather;
    // the caller's embedding indexes (bert_hip_index_create), freed with the context before the gather and the engines
    std::vector<bert_hip_index *> indexes;
    // the caller's sparse indexes (bert_hip_sparse_index_create), freed with the context in the same place
    std::vector<bert_hip_sparse_index *> sparse_indexes;
    // the caller's token indexes (bert_hip_token_index_create), freed with the context in the same place
    std::vector<bert_hip_token_index *> token_indexes;

    bert_hip::Engine *engine() const { return engines.empty() ? nullptr : engines[0].get(); }
    ~bert_ctx() {
        for (bert_hip_index *ix : indexes) delete ix;
        for (bert_hip_sparse_index *ix : sparse_indexes) delete ix;
        for (bert_hip_token_index *ix : token_indexes) delete ix;
    }
};

namespace bert_hip {

// The devices a list names, of n_devices visible ones: "all", or ordinals separated by commas (a trailing comma is accepted);
// no list (null or empty) is the caller's current device.  false + err for an ordinal that cannot be parsed, is out of range
// or is named twice.
bool parse_device_list(const char *list, int n_devices, int current, std::vector<int> &devs, std::string &err);
// the devices a new context spreads over: BERT_HIP_DEVICES, else BERT_HIP_DEVICE (the single-device spelling of earlier builds,
// an alias for a list of one), else the calling thread's current device
bool context_devices(std::vector<int> &devs, std::string &err);

// bert_load_from_file / bert_hip_load_tokenizer: nullptr after a line on stderr
bert_ctx *load_impl(const char *fname, bool tokenizer_only);

}  // namespace bert_hip
