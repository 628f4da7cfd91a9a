// profiler.h — per-kernel times of the forward pass (bert_hip_profile_enable / bert_hip_profile_report): an event pair per
// launch, or ("profile_replay") K repeats of one kernel between one pair; launch counts per mat-mul kernel family.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "kernels.h"

namespace bert_hip {

class LaunchProfiler {
public:
    LaunchProfiler() = default;
    LaunchProfiler(const LaunchProfiler &) = delete;
    LaunchProfiler &operator=(const LaunchProfiler &) = delete;
    ~LaunchProfiler();                                        // (the owner has set the device and drained it)

    void enable(bool on) { profiling_ = on; }
    bool enabled() const { return profiling_; }
    // "<kernel name>:<K>" (see timed()), "" switches back to an event pair per launch
    void set_replay(const std::string &value);
    void begin_pass() { replay_done_ = false; }
    // a mat-mul launch of a kernel family ("family:gemm256_q4" ...); not counted while one kernel is replayed
    void count_family(const std::string &family) { if (profiling_ && replay_name_.empty()) families_[family] += 1; }
    // runs f (which launches on s), timed when profiling is on
    template <class F> void timed(const char *name, double flops, hipStream_t s, F &&f) {
        if (!profiling_) f();
        else if (!replay_name_.empty()) replay(name, flops, s, f);
        else {
            // an event pair attached to the dispatch itself (kernels.h BERT_LAUNCH): an upper bound of the kernel's time in the pass
            Pending p{name, get_event(), get_event(), flops, 1};
            LaunchTiming lt{p.a, p.b, 0};
            tl_launch_timing = &lt;
            f();
            tl_launch_timing = nullptr;
            // exactly one launch carries the pair; anything else (a launcher that returned early: stale timestamps of pooled events;
            // several launches: only the last one measured) is not a sample
            if (lt.launches == 1) pending_.push_back(p);
            else { ev_pool_.push_back(p.a); ev_pool_.push_back(p.b); }
        }
    }
    // one line per kernel, "<name> <launches> <ms> <flops per launch>", then one per family, "<family> <launches> 0 0"; clears
    // both.  The caller has set the device and waited for it.
    std::string report();

private:
    struct Pending { const char *name; hipEvent_t a, b; double flops; int launches; };
    struct KernelStat { int launches = 0; double ms = 0.0; double flops = 0.0; };
    hipEvent_t get_event();
    template <class F> void replay(const char *name, double flops, hipStream_t s, F &&f) {
        // replay form ("profile_replay" = "<kernel>:<K>"): the pass runs untimed; behind the FIRST launch of the named kernel
        // the same launch is repeated K times between ONE event pair — the pair's own cost (tens of microseconds around a
        // sub-millisecond kernel) is spread over K launches, so launches x average cannot exceed the step they belong to.
        // Kernels that work in place see their own output as input in the repeats: the pass's results are not to be used.
        f();
        if (replay_done_ || replay_name_ != name) return;
        replay_done_ = true;
        warn_replay();
        Pending p{name, get_event(), get_event(), flops * replay_k_, replay_k_};
        (void)hipEventRecord(p.a, s);
        for (int k = 0; k < replay_k_; ++k) f();
        (void)hipEventRecord(p.b, s);
        pending_.push_back(p);
    }
    static void warn_replay();

    bool profiling_ = false;
    std::vector<hipEvent_t> ev_pool_;
    std::string replay_name_;
    int replay_k_ = 10;
    bool replay_done_ = false;
    std::vector<Pending> pending_;
    std::map<std::string, KernelStat> stats_;
    std::map<std::string, int> families_;
};

}  // namespace bert_hip
