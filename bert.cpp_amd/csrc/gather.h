// gather.h — a packed batch over all engines of a context (contiguous token-balanced shards, one host thread per device), and
// on top of it the device-resident result of bert_hip_eval_packed_gather: every device ends up with the whole
// [n_sentences][n_embd] matrix, exchanged by RCCL super-batch by super-batch under the next super-batch's compute.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "multi_device.h"

namespace bert_hip {

using Engines = std::vector<std::unique_ptr<Engine>>;

// One packed batch over the engines: every shard's embeddings written straight into the caller's rows (embeddings), or,
// d_dst: into the shard's device buffer d_dst[device].  Host-row batches of fewer than 2048 tokens per device use fewer
// devices (a launch sequence costs ~50 us whatever the size).  workers: the context's threads, or null (one device after the
// other).  0, or an engine's error code and err; a worker's exception arrives as -9.  pool_mode: kernels.h POOL_*, what every shard
// ends by (-1: each engine reads its options).
int eval_packed_all_devices(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int B,
                            float *embeddings, std::string &err, float *const *d_dst = nullptr, int pool_mode = -1);

// Grouped pooling (bert_hip.h "long texts"; Engine::eval_packed_grouped_host) over the engines: one row per group of consecutive
// sentences into embeddings (host, [n_groups][H]) or d_embeddings (the FIRST device's memory).  One device: the sentences' raw rows
// never leave it.  Several: the raw rows come through the sharded host path above into a host buffer, are uploaded to the first
// device and pooled there — per-group bits do not depend on the number of devices.
int eval_packed_grouped_all_devices(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int B,
                                    const int32_t *group_cu, int n_groups, float *embeddings, float *d_embeddings, std::string &err);

// SUPER-BATCHES ("one gather per super-batch, overlapped with the next super-batch's compute"): a gather call is
// cut into runs of sentences.  runs[k] .. runs[k + 1]: the sentences of run k (runs[0] = 0, the last entry n_sentences); a run
// is closed in front of the first sentence with which it would hold more than tokens_per_run tokens, so a run of several
// sentences never exceeds that, and a longer sentence is a run of its own.
void gather_runs(const int32_t *cu, int n_sentences, long long tokens_per_run, std::vector<int> &runs);

// The state of bert_hip_eval_packed_gather, owned by the context.  Lifetime rules, all kept here:
//  * the destructor drains and destroys the exchange streams before the shard buffers and the communicator go; the context
//    declares the gather behind its engines, so all this happens while the engines (devices, streams) are still there;
//  * in run, every fallible preparation (buffers, streams, events, the communicator) happens before any rank enters RCCL: a
//    rank that fails between its peers' collectives leaves them waiting in a collective that never completes;
//  * a failure after the first exchange has been issued does not return while earlier exchanges still write the gathered
//    matrices and read the shard buffers: every exchange and engine stream is drained first.
class EmbeddingGather {
public:
    EmbeddingGather() = default;
    EmbeddingGather(const EmbeddingGather &) = delete;
    EmbeddingGather &operator=(const EmbeddingGather &) = delete;
    ~EmbeddingGather();

    // tokens per device and super-batch (option "gather_super_tokens"; 0: four device chunks)
    int super_tokens = 0;
    // test knob (option "test_rccl_single"): a single device runs the exchange step on a 1-rank communicator
    bool rccl_single = false;
    // (made at load on a multi-device context, so that the first call does not pay for it)
    RcclGather rccl;

    // n_sentences validated sentences -> d_embeddings[d]: the [n_sentences][n_embd] matrix on device d (this object's memory,
    // valid until the next call).  Blocking.  false + err on a failure.
    bool run(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int n_sentences,
             float **d_embeddings, std::string &err);

private:
    void drain(const Engines &engines);
    // per device: two shard buffers (super-batch k + 1 is computed into one while the exchange of super-batch k reads the
    // other) and the gathered matrix; grow-only
    std::vector<std::unique_ptr<DevBuf>> shard_out_, gathered_;
    // the exchange's own stream per device and an event per (device, shard buffer): "the exchange that read this buffer is done"
    std::vector<hipStream_t> xstream_;
    std::vector<hipEvent_t> xdone_;
    std::vector<int> devs_;             // the engines' devices
};

}  // namespace bert_hip
