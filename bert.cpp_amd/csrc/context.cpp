// context.cpp — see context.h.  Reference behaviour mirrored here: bert_load_from_file, reference bert.cpp:331-694.
#include "context.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <system_error>
#include <thread>

#include "model_file.h"

namespace bert_hip {

bool parse_device_list(const char *list, int n_devices, int current, std::vector<int> &devs, std::string &err) {
    devs.clear();
    if (!list || !*list) {
        devs.push_back(current < 0 || current >= n_devices ? 0 : current);
    } else if (strcmp(list, "all") == 0) {
        for (int d = 0; d < n_devices; ++d) devs.push_back(d);
    } else {
        for (const char *p = list; *p;) {
            char *end = nullptr;
            const long d = strtol(p, &end, 10);
            if (end == p) { err = std::string("BERT_HIP_DEVICES: cannot parse '") + list + "'"; return false; }
            if (d < 0 || d >= n_devices) { err = "BERT_HIP_DEVICES: ordinal " + std::to_string(d) + " out of range"; return false; }
            devs.push_back((int)d);
            p = *end == ',' ? end + 1 : end;
        }
    }
    if (devs.empty()) { err = "BERT_HIP_DEVICES names no device"; return false; }
    for (size_t i = 0; i < devs.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (devs[i] == devs[j]) { err = "BERT_HIP_DEVICES lists device " + std::to_string(devs[i]) + " twice"; return false; }
    return true;
}

bool context_devices(std::vector<int> &devs, std::string &err) {
    int ndev = 0, cur = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        err = "no HIP device available (this library needs an AMD GPU; there is no CPU fallback)";
        return false;
    }
    const char *list = getenv("BERT_HIP_DEVICES");
    if (!list || !*list) list = getenv("BERT_HIP_DEVICE");
    if (hipGetDevice(&cur) != hipSuccess) cur = 0;
    return parse_device_list(list, ndev, cur, devs, err);
}

bert_ctx *load_impl(const char *fname, bool tokenizer_only) {
    const char *q = getenv("BERT_HIP_QUIET");
    const bool quiet = q && *q && *q != '0';
#define ME "bert_load_from_file: "
    if (!quiet) printf(ME "loading model from '%s' - please wait ...\n", fname);
    ModelFile mf;
    std::string err;
    if (!mf.load(fname, tokenizer_only, err)) {
        fprintf(stderr, ME "%s\n", err.c_str());
        return nullptr;
    }
    if (!quiet) {
        printf(ME "n_vocab = %d\n" ME "n_max_tokens   = %d\n" ME "n_embd  = %d\n" ME "n_intermediate  = %d\n"
               ME "n_head  = %d\n" ME "n_layer = %d\n" ME "f16     = %d\n",
               mf.hp.n_vocab, mf.hp.n_max_tokens, mf.hp.n_embd, mf.hp.n_intermediate, mf.hp.n_head, mf.hp.n_layer, mf.hp.f16);
        if (mf.legacy_q4)
            printf(ME "legacy q4 layout (f32 block scales, 20 / 24-byte blocks): re-blocked at load, scales rounded to f16\n");
    }
    std::unique_ptr<bert_ctx> ctx(new bert_ctx);
    ctx->hp = mf.hp;
    ctx->tok.build(std::move(mf.vocab));
    ctx->tok.quiet = quiet;           // BERT_HIP_QUIET also drops the reference's per-byte "unknown token" stderr lines
    ctx->rel_bias = mf.rel_bias;
    if (mf.rel_bias) {
        // an MPNet file: its texts are <s> ... </s>.  (Every BERT file keeps 101 / 102 whatever its vocabulary holds.)
        ctx->tok.cls_id = ctx->tok.find("<s>");
        ctx->tok.sep_id = ctx->tok.find("</s>");
        if (ctx->tok.cls_id < 0 || ctx->tok.sep_id < 0) {
            fprintf(stderr, ME "the model has a relative position bias (%s) but its vocabulary has no '%s' entry\n", REL_BIAS_NAME,
                    ctx->tok.cls_id < 0 ? "<s>" : "</s>");
            return nullptr;
        }
    }
    ctx->texts.tok = &ctx->tok;
    ctx->texts.n_max_tokens = mf.hp.n_max_tokens;
    if (tokenizer_only) return ctx.release();
    std::vector<int> devs;
    if (!context_devices(devs, err)) {
        fprintf(stderr, ME "%s\n", err.c_str());
        return nullptr;
    }
    int caller_device = 0;
    const bool have_caller_device = hipGetDevice(&caller_device) == hipSuccess;
    // the replicas are built side by side (each upload is host-bound: repacking + H2D), one thread per extra device
    std::vector<Engine *> made(devs.size(), nullptr);
    std::vector<std::string> errs(devs.size());
    {
        std::vector<std::thread> builders;
        auto build = [&](size_t i) {
            try { made[i] = Engine::create(mf, devs[i], errs[i]); }
            catch (const std::exception &e) { errs[i] = e.what(); }
            catch (...) { errs[i] = "unknown exception"; }
        };
        for (size_t i = 1; i < devs.size(); ++i) {
            try { builders.emplace_back(build, i); } catch (const std::system_error &) { build(i); }
        }
        build(0);
        for (auto &th : builders) th.join();
    }
    if (have_caller_device) (void)hipSetDevice(caller_device);   // loading leaves the caller's current device alone
    bool ok = true;
    for (size_t i = 0; i < devs.size(); ++i) {
        if (made[i]) ctx->engines.emplace_back(made[i]);
        else if (ok) { fprintf(stderr, ME "%s\n", errs[i].c_str()); ok = false; }
    }
    if (!ok) return nullptr;                              // (the engines made so far are freed with the context)
    if (devs.size() > 1) {
        ctx->workers.reset(new ShardWorkers((int)devs.size() - 1));
        // the communicator of the embedding gather is made now, not inside the first timed call
        if (!ctx->gather.rccl.init(devs, err) && !quiet)
            fprintf(stderr, ME "RCCL is not available (%s): bert_hip_eval_packed_gather will fail, everything else works\n", err.c_str());
        if (have_caller_device) (void)hipSetDevice(caller_device);
    }
    if (!quiet)
        printf(ME "model size = %8.2f MB / num tensors = %zu (HBM-resident on %zu HIP device%s, first %d)\n",
               mf.total_tensor_bytes / 1024.0 / 1024.0, mf.tensors.size(), devs.size(), devs.size() == 1 ? "" : "s", devs[0]);
#undef ME
    return ctx.release();
}

}  // namespace bert_hip
