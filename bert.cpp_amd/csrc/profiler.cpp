// profiler.cpp — see profiler.h.
#include "profiler.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace bert_hip {

LaunchProfiler::~LaunchProfiler() {
    for (auto ev : ev_pool_) (void)hipEventDestroy(ev);
    for (auto &p : pending_) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
}

void LaunchProfiler::set_replay(const std::string &value) {
    const size_t c = value.rfind(':');
    replay_name_ = c == std::string::npos ? value : value.substr(0, c);
    replay_k_ = c == std::string::npos ? 10 : std::max(1, atoi(value.c_str() + c + 1));
}

hipEvent_t LaunchProfiler::get_event() {
    hipEvent_t ev;
    if (!ev_pool_.empty()) { ev = ev_pool_.back(); ev_pool_.pop_back(); }
    else (void)hipEventCreate(&ev);
    return ev;
}

// (in-place kernels run on their own output from here on: this pass's embeddings are NOT results — bench.py restores
// its output buffer; say so once for anybody else who turns the option on)
void LaunchProfiler::warn_replay() {
    static bool warned = false;
    if (!warned && !getenv("BERT_HIP_QUIET")) { warned = true; fprintf(stderr, "bert_hip: profile_replay is active: the embeddings of profiled passes are not valid results\n"); }
}

std::string LaunchProfiler::report() {
    for (auto &p : pending_) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            KernelStat &st = stats_[p.name];
            st.launches += p.launches; st.ms += ms; st.flops += p.flops;
        }
        ev_pool_.push_back(p.a); ev_pool_.push_back(p.b);
    }
    pending_.clear();
    std::string out;
    char line[256];
    for (auto &kv : stats_) {
        snprintf(line, sizeof(line), "%s %d %.6f %.6e\n", kv.first.c_str(), kv.second.launches, kv.second.ms,
                 kv.second.launches ? kv.second.flops / kv.second.launches : 0.0);
        out += line;
    }
    stats_.clear();
    for (auto &kv : families_) {
        snprintf(line, sizeof(line), "%s %d 0 0\n", kv.first.c_str(), kv.second);
        out += line;
    }
    families_.clear();
    return out;
}

}  // namespace bert_hip
