// model_kernel.hip — ONE launch for all encoder layers of a batch (f16 images, H = 256 / 384, d_head 32, sentences of at most
// 128 tokens) plus the pooling: reference bert.cpp:816-913, the whole loop over layers and what follows it.  Two forms: FULL
// windows (every sentence exactly 128 tokens: a window is a sentence is a 128-token block) and RAGGED ones (whole sentences
// with at most 128 tokens between them: the layer-tail phase runs on the window's rows of the packed batch).
//
// Why: with one kernel per layer half (qkv_attention2, layer_tail) a 256-sentence step is ONE workgroup per CU per launch,
// all 256 in lockstep — everybody's load burst (ctx + x: 48 MB at the HBM limit), everybody's compute, everybody's store
// burst, twelve times per forward pass; two free-running half-batch lanes already measure +4-6 % (tools/dual_lane_probe.py),
// but a call has to join its lanes.  A window's tokens depend on no other window's: here a workgroup carries ITS window
// through every layer — window-kernel phase (Q|K|V projection + attention), layer-tail phase (out-projection + LN + FFN + LN),
// the two kernels' bodies unchanged (same arithmetic, same bits: tested) — and nothing ever puts the workgroups back in step.
// The hand-overs (ctx from the attention waves to the tail, x from the tail to the next layer's projection waves) are plain
// global stores and loads of the SAME workgroup: 96 KiB each, behind a workgroup-scope fence (one L1 per CU, shared by the
// workgroup's waves: no invalidate needed outside threadgroup-split mode); on full windows x ALSO crosses in registers and ctx crosses
// ONLY on chip, in registers and through LDS (the layer loop below), so neither phase waits for a round trip of its own data, and no ctx
// is stored at all; what the next tail needs of x as its residual crosses through a scratch workspace in LANE ORDER (LayerNorm 2's
// result fragments as they are: the layer loop below), so the full form stores rows of x after its last layer only — and loads none
// before: its embedding kernel writes that workspace in lane order for layer 0 (embed_ln_lanes_kernel, misc_kernels.hip).  The global
// hand-overs (the ragged form's both, the full form's residual fragments) do NOT stay inside the XCD's L2: 256
// workgroups x 192 KiB = 48 MiB per layer against 32 MiB of L2, and every store leaves the L2 towards the fabric anyway —
// measured 313 MB written and 1.06 GB of fabric traffic per launch with both edges through memory (profiles/r3_pmc.txt), 164 MB and
// 0.52 GB for the full form with x stored as rows by every layer (profiles/traffic.json), absorbed by the Infinity Cache at
// about 1.3 TB/s: far from a limit, but not free.  What the single launch removes is the lockstep, not the bytes.
// Full form only: the kernel trusts n_tokens = 128 n_sentences to mean "every sentence is exactly 128 tokens"; that holds
// whenever the caller's max_len promise (<= 128) does.  A batch that breaks it is flagged by the pooling guard (status word),
// and the rows of sentences sharing a 128-token block with the offender are not meaningful (include/bert_hip.h).
//
// Both bodies keep their own LDS layout (160 KiB each, used one after the other) and register budget (256 per wave).  This
// translation unit is compiled with the flags of both (Makefile): -fno-slp-vectorize (qkv_attention2) and
// -structurizecfg-skip-uniform-regions (layer_tail).
#define BERT_HIP_PHASES_ONLY
#include "qkv_attention2.hip"
#include "layer_tail.hip"
#undef BERT_HIP_PHASES_ONLY
#include "pool_normalize.h"

#include <cstdlib>

namespace bert_hip {

#ifdef BERT_HIP_MODEL_TIMELINE      // (tuning aid: tools/variant.sh tl "-DBERT_HIP_MODEL_TIMELINE")
// phase boundaries of every workgroup on the constant 100 MHz counter: [0] start, [1 + 2 l] window phase of layer l done, [2 + 2 l] its tail
// phase done, [1 + 2 L] pooled
static __device__ unsigned long long g_tl_model[1024 * 32];
#define MK_STAMP(i) do { const int mk_i = (i); if (threadIdx.x == 0 && mk_i < 32) g_tl_model[(blockIdx.x & 1023) * 32 + mk_i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define MK_STAMP(i) do { } while (0)
#endif

namespace {

struct ModelLayerArgs {              // what differs from layer to layer
    const half_t *wqkv, *wo, *w1p, *w2p;
    const float *bqkv, *bo, *g1, *be1, *b1, *b2, *g2, *be2;
};
struct ModelArgs {
    half_t *x, *ctx;                 // [T][H] hidden state (RAGGED in: embeddings + LN; out: the last layer's output), attention context
    const int32_t *cu;
    const int2 *groups;              // RAGGED: per window {first sentence, count} (qkv_attention2.hip), or nullptr: one sentence per window
    const int *n_groups;             // RAGGED: device word holding the number of windows (the grid is an upper bound), or nullptr
    int n_layer, n_head, n_sent, I, slot_mask;      // slot_mask: the windows' place granularity - 1 (Qkv2Args)
    float *pooled;                   // [n_sent][H] f32: the sentences' pooled, normalised rows (the workgroup pools its window itself), or nullptr
    int *status;                     // pooling's status word (a sentence outside [1, max_len])
    int max_len, pool_mode;          // pool_mode: kernels.h POOL_CLS | POOL_RAW, read by the epilogue alone (POOL_MODES forms)
    ModelLayerArgs layer[MODEL_MAX_LAYERS];
    half_t *xres;                    // FULL windows: [T][H] in lane order (layer_tail_body's XRES_IN / XRES_OUT) — in: embeddings + LN, then the
                                     // residual x between two tails; behind everything else: the ragged form, which ignores it, finds its arguments where they were
};

}  // namespace

// RAGGED: windows of whole sentences with up to 128 tokens between them (the window phase's slots: every sentence starts at a
// multiple of 16), whose rows of x / ctx are tok0 .. tok0 + rows - 1 of the packed batch: the layer-tail phase runs on those.
// POOL_MODES: the epilogue pools as m.pool_mode says; else by the default rule, mean + L2 normalisation, as a constant.  The
// layer loop is the same text in both, but with a run-time mode in the epilogue the compiler schedules the loop differently and
// picks other scalar registers in it (no register more, no spill more: profiles/pooling_resources.txt): the default mode keeps a
// form of its own, whose machine code is the kernel's from before the modes existed.
template <int NT, bool RAGGED, bool POOL_MODES>
__global__ __launch_bounds__(512, 2) void model_kernel(ModelArgs m) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int window = (int)blockIdx.x;              // full windows: = sentence = 128-token block
    int tok0 = window * 128, rows = 128, first = window, count = 1;
    if constexpr (RAGGED) {
        if (m.groups) {
            if (m.n_groups && window >= *m.n_groups) return;
            const int2 g = m.groups[window];
            first = g.x; count = g.y;
        }
        if (count <= 0 || first >= m.n_sent) return;
        tok0 = m.cu[first];
        // (a sentence longer than a window breaks the caller's promise: its rows behind the 128th are not computed — it is the
        // one that gets a NaN row from the length guard of the pooling kernel)
        rows = min(m.cu[first + count] - tok0, 128);
    }
    // The thread id is REBUILT per phase from the wave's index (a scalar register) and the lane count: with threadIdx.x itself
    // the compiler hoists both phases' lane-dependent address arithmetic out of the layer loop — eighty registers' worth —
    // and spills it; even one vector register alive across the phases is one more than the layer tail has (a scratch reload
    // among its hand-counted LDS-DMA pieces would break their vmcnt arithmetic).
    const int wave_index = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    auto thread_id = [&]() __attribute__((always_inline)) {
        int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), w = wave_index;
        asm volatile("" : "+v"(ln), "+s"(w));
        return w * 64 + ln;
    };
    MK_STAMP(0);
    const int n_layer = rows > 0 ? m.n_layer : 0;    // (a window of empty sentences: nothing to compute, NaN rows from the pooling below)
    // A phase = the kernel's body on this workgroup's window.  Full windows (!RAGGED) tell the window phase so (FULL: its slots are the
    // block's tokens, no look at cu) and, from the second layer on, hand it the hidden state in registers (XREGS / HANDOVER below).
    // The first layer has nobody's registers to start from: its window phase takes the same fragments from m.xres, where the embedding kernel
    // wrote the hidden state in lane order (XLANES: xf == nullptr in the full form).
    auto window_phase = [&](const ModelLayerArgs &L, auto first_tag, const f16x8 *xf, f16x8 *cf) __attribute__((always_inline)) {
        const int tid = thread_id();
        Qkv2Args q;
        q.x = m.x; q.w = L.wqkv; q.qs = nullptr; q.sc = nullptr; q.bias = L.bqkv; q.cu = m.cu; q.groups = RAGGED ? m.groups : nullptr; q.n_groups = nullptr;
        q.out = m.ctx; q.n_head = m.n_head; q.n_sent = m.n_sent; q.spw = 1; q.slot_mask = m.slot_mask;
        constexpr bool FIRST = decltype(first_tag)::value;
        qkv_attention2_body<2 * NT, NT, GW_F16, !RAGGED, !RAGGED, !RAGGED, !RAGGED && FIRST>(q, smem, window, tid, xf, cf, RAGGED ? nullptr : m.xres);
    };
    auto tail_phase = [&](const ModelLayerArgs &L, f16x8 (&xf)[8 * NT], const f16x8 *cf, [[maybe_unused]] const bool lane_out) __attribute__((always_inline)) {
        const int tid = thread_id();
        TailArgs t;
        t.ctx = m.ctx; t.x = m.x; t.wo = L.wo; t.w1p = L.w1p; t.w2p = L.w2p;
        t.wo_qs = t.w1_qs = t.w2_qs = nullptr; t.wo_sc = t.w1_sc = t.w2_sc = nullptr;
        t.bo = L.bo; t.g1 = L.g1; t.be1 = L.be1; t.b1 = L.b1; t.b2 = L.b2; t.g2 = L.g2; t.be2 = L.be2; t.out = m.x; t.I = m.I;
        if constexpr (RAGGED) layer_tail_body<NT, GW_F16, true, false, false>(t, smem, tok0, rows, tid, xf, cf);
        else layer_tail_body<NT, GW_F16, false, true, true, true, true>(t, smem, tok0, rows, tid, xf, cf, m.xres, lane_out);
    };
    // Phase edge: everything the phase stored (ragged windows: ctx by the attention waves; x by all waves) is visible to the workgroup, every
    // LDS access of the phase has returned (the next phase's first DMA pieces overwrite what the others were reading).  On full windows
    // the window -> tail edge has no fresh global store to wait for (ctx crosses on chip, below): there the wait and the barrier order the
    // attention waves' LDS writes of the last head's fragments before the tail's reads, and the fence keeps the compiler from moving
    // either across it.
    auto hand_over = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    if constexpr (RAGGED) {
        for (int l = 0; l < n_layer; ++l) {
            f16x8 none[8 * NT];                          // (no register hand-over: a ragged window's tail rows are packed, its slots are not)
            window_phase(m.layer[l], std::false_type{}, nullptr, nullptr);
            hand_over();
            MK_STAMP(1 + 2 * l);
            tail_phase(m.layer[l], none, nullptr, false);
            hand_over();
            MK_STAMP(2 + 2 * l);
        }
    } else {
        // Full windows: the tail's D waves 4..7 end with the rows of x they have just normalised in registers, and the same waves, as
        // the next layer's projection waves, start from those rows — same lanes, same tokens, the f16 values that are stored: LayerNorm 2
        // hands them over as operand fragments (layer_tail_body's HANDOVER) and the window phases of layers 1 .. L-1 load no x at all
        // (the residual of the next tail and the pooling still read what is stored: below; layer 0's load theirs from m.xres).  The loop is rotated — layer 0's window phase in front,
        // then tail(l) -> window(l + 1) per turn — so that the fragments are born and consumed inside ONE turn: declared outside, the
        // U waves' path (which does not write them) would carry 96 registers round the loop and through the tail.
        //
        // The other edge, window -> tail, crosses on chip too: no ctx is stored and none is loaded (m.ctx is the ragged form's).  Attention wave a
        // (0..3) and the tail's U wave of pair a are the same wave with the same tokens: it keeps every head's rounded result as the out-projection's
        // operand fragments `cf` (qkv_attention2_body's CTXREGS) and the tail starts from them (layer_tail_body's CTXREGS).  The pair's D wave
        // (4 + a, a projection wave in the window phase) gets the same fragments through LDS.  Map of the edge (KiB; H = 384 | 256):
        //     window phase          ring [0, 108 | 72)   Q/K/V copy 0 [108, 132.25 | 72, 96.25)   copy 1 (the last head's) behind it
        //     exchange, older heads [0, 96 | 64): block b at 8 NT b, fragment q of lane l at + q + 16 l bytes.  Written behind the barrier that
        //                           publishes the last head — the ring is dead, and in this form that barrier waits for the dead prefetches as
        //                           well — and read by the D waves, idle by then, behind one more barrier [X] while the last head is attended
        //     last two heads' four  ctx_edge_offset = [96, 112 | 80, 96): block b at + 4 b; dead ring and dead copy 0 | dead copy 0 in the window phase;
        //                           the tail's GELU area | third slot of ringD, which get their first bytes behind the tail's first barrier.  The
        //                           attention wave writes them in front of [X] and at the end of the window phase (it has no registers to keep
        //                           them through the last head's attention); both waves of the pair read them in the tail's prologue
        //     tail phase prologue   DMA into ringU / ringD slots 0, 1 = [0, 32) and [48, 80), parameters behind 128: all of it behind the
        //                           edge's barrier, when every D wave holds the exchange area's fragments in registers (its reads are
        //                           waited for inside the window phase)
        // `cf` is written by every wave in the window phase and read by every wave in the tail, so it lives across the back edge for what it
        // is; where no window phase follows it is named as written, or the last tail would carry the fragments it has consumed.
        //
        // The residual x of tail(l + 1) is what LayerNorm 2 of tail(l) wrote, and only this workgroup reads it before the pooling: between two
        // tails it crosses in LANE ORDER through m.xres (layer_tail_body's XRES_IN / XRES_OUT: D's result fragments as they are, 1 KiB per
        // wave-instruction on both sides, no staging in LDS, no barriers around it, no row stores), behind the same two phase edges as before.
        //     layers 0 .. L-2:  lane order in and out: m.x is neither read nor written
        //     layer L-1:        lane order in, rows out (the pooling below and the caller read m.x); L = 1 is this line alone
        // Layer 0 is a layer like the others: the embedding kernel of this route (misc_kernels.hip embed_ln_lanes_kernel) writes the hidden
        // state into m.xres in lane order and no rows at all, tail 0 loads its residual like every tail, and window phase 0 starts from the
        // same fragments (qkv_attention2_body's XLANES: 8 NT contiguous KiB per projection wave instead of 8 NT row-major fragments).  So the
        // full form reads NO m.x before its last tail has written it.  Every fragment a tail loads was stored in the same pass, by the
        // embedding kernel or by the tail before it in this launch (tests: x, the scratch and everything else poisoned with NaNs).
        f16x8 cf[8 * NT];
        if (n_layer > 0) window_phase(m.layer[0], std::true_type{}, nullptr, cf);
        for (int l = 0; l < n_layer; ++l) {
            hand_over();
            MK_STAMP(1 + 2 * l);
            f16x8 xf[8 * NT];
            tail_phase(m.layer[l], xf, cf, l + 1 < n_layer);
            hand_over();
            MK_STAMP(2 + 2 * l);
            if (l + 1 < n_layer) window_phase(m.layer[l + 1], std::false_type{}, xf, cf);
            else {
#pragma unroll
                for (int q = 0; q < 8 * NT; ++q) asm volatile("" : "=v"(cf[q]));
            }
        }
    }
    // ---- mean-pool + L2 normalise (or what m.pool_mode asks for) of the window's sentences (pool_normalize.h: the pooling kernel's
    // body and bits), while the other workgroups are still in their layers: the rows were written by this workgroup and sit in the L2
    if (m.pooled) {
        const int tid = thread_id();
        for (int j = 0; j < count; ++j) {
            const int b = first + j, t0 = m.cu[b];
            int n = m.cu[b + 1] - t0;
            // (the full-window form computed rows 128 b .. 128 b + 127 as ONE sentence: in a batch that has this shape only by the
            // sum of its lengths — somebody longer than max_len = 128, somebody shorter — a sentence that is not exactly that block
            // gets the NaN row and the status word of the length guard instead of numbers made of its neighbours' tokens)
            if (!RAGGED && (t0 != tok0 || n != 128)) n = -1;
            if constexpr (POOL_MODES) pool_normalize_sentence(m.x, t0, n, b, 128 * NT, m.max_len, m.status, m.pooled, (float *)smem, tid, tid < 256, m.pool_mode);
            else pool_normalize_sentence<false, false>(m.x, t0, n, b, 128 * NT, m.max_len, m.status, m.pooled, (float *)smem, tid, tid < 256);
            __syncthreads();                                  // (the next sentence reuses the partial rows)
        }
    }
    MK_STAMP(1 + 2 * n_layer);
}

// full: every sentence exactly 128 tokens (T = 128 B: the specialised form); otherwise windows of whole sentences — the caller's
// list (`groups`), or one sentence per window when the promised max_len leaves room for no second one
bool model_kernel_supported(const GemmWeight &Wqkv, const GemmWeight &Wo, const GemmWeight &W1, const GemmWeight &W2, int n_layer,
                            int n_head, int d_head, int max_len) {
    const int H = n_head * d_head;
    return n_layer <= MODEL_MAX_LAYERS && (H == 256 || H == 384) && max_len >= 1 && max_len <= 128 &&
           Wqkv.type == GW_F16 && Wo.type == GW_F16 && qkv_attention2_supported(Wqkv, n_head, d_head, max_len) && layer_tail_supported(Wo, W1, W2);
}

void launch_model_kernel(const ModelLayerWeights *layers, int n_layer, half_t *x, half_t *ctx, half_t *xres, const int32_t *cu_seqlens, int n_sentences,
                         int n_tokens, const int2 *groups, int n_groups, const int *n_groups_dev, int n_head, float *pooled, int max_len,
                         int *status, int pool_mode, int slots, hipStream_t stream) {
    ModelArgs m;
    m.pooled = pooled; m.status = status; m.max_len = max_len; m.pool_mode = pool_mode;
    m.x = x; m.ctx = ctx; m.xres = xres; m.cu = cu_seqlens; m.groups = groups; m.n_groups = n_groups_dev;
    m.n_layer = n_layer; m.n_head = n_head; m.n_sent = n_sentences; m.I = layers[0].W1->N; m.slot_mask = slots - 1;
    for (int l = 0; l < n_layer; ++l) {
        const ModelLayerWeights &s = layers[l];
        ModelLayerArgs &d = m.layer[l];
        d.wqkv = s.Wqkv->w16; d.wo = s.Wo->w16; d.w1p = s.W1->w16p; d.w2p = s.W2->w16p;
        d.bqkv = s.bqkv; d.bo = s.bo; d.g1 = s.g1; d.be1 = s.be1; d.b1 = s.b1; d.b2 = s.b2; d.g2 = s.g2; d.be2 = s.be2;
    }
    const int H = layers[0].W1->K, KT = H / 64, GB = KT / 2;
    const size_t lds_q = (size_t)3 * GB * Q2_TILE + 2 * (2 * Q2_WIN * 64 + 32 * Q2_VT_LD * 2) + (size_t)2 * H * sizeof(float);
    const size_t lds = std::max(lds_q, layer_tail_lds(H, m.I));
    const bool full = (long long)n_sentences * 128 == n_tokens;      // (with no sentence over 128 tokens: every window is one whole sentence)
    // (the full form keeps two context fragments per head in a register array sized by H: model_kernel_supported's d_head = 32)
    if (n_head * 32 != H) { fprintf(stderr, "launch_model_kernel: n_head %d x 32 != H %d\n", n_head, H); abort(); }
    const int grid = full || !groups ? n_sentences : n_groups;
    static DeviceFlags configured[8];
    auto go = [&](auto kernel, int which) {
        configure_once(configured[which], [&] { (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
        BERT_LAUNCH(kernel, dim3(grid), dim3(512), lds, stream, m);
#ifdef BERT_HIP_MODEL_TIMELINE
        static int shots = 0;
        if (grid >= 256 && shots++ == 30) {
            (void)hipDeviceSynchronize();
            static unsigned long long h[1024 * 32];
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tl_model), sizeof(h));
            const int nw = grid < 1024 ? grid : 1024, ns = 2 + 2 * n_layer;
            unsigned long long t0 = ~0ull;
            for (int w = 0; w < nw; ++w) t0 = h[w * 32] < t0 ? h[w * 32] : t0;
            // per stamp: min / mean / max over the workgroups of (stamp - earliest start), in microseconds (100 MHz counter)
            fprintf(stderr, "model_kernel timeline, %d workgroups (us after the first workgroup's start: min mean max):\n", nw);
            for (int i = 0; i < ns; ++i) {
                double lo = 1e30, hi = 0, sum = 0;
                for (int w = 0; w < nw; ++w) { const double v = (double)(h[w * 32 + i] - t0) * 0.01; lo = v < lo ? v : lo; hi = v > hi ? v : hi; sum += v; }
                fprintf(stderr, "  stamp %2d: %8.2f %8.2f %8.2f\n", i, lo, sum / nw, hi);
            }
            // per phase: mean duration over workgroups
            fprintf(stderr, "  mean phase durations (window, tail) per layer:");
            for (int l = 0; l < n_layer; ++l) {
                double a = 0, b = 0;
                for (int w = 0; w < nw; ++w) { a += (double)(h[w * 32 + 1 + 2 * l] - h[w * 32 + 2 * l]) * 0.01; b += (double)(h[w * 32 + 2 + 2 * l] - h[w * 32 + 1 + 2 * l]) * 0.01; }
                fprintf(stderr, " (%.1f, %.1f)", a / nw, b / nw);
            }
            fprintf(stderr, "\n  mean end per XCD:");
            for (int x = 0; x < 8; ++x) {
                double e = 0; int c = 0;
                for (int w = x; w < nw; w += 8) { e += (double)(h[w * 32 + ns - 1] - t0) * 0.01; ++c; }
                fprintf(stderr, " %.1f", e / c);
            }
            fprintf(stderr, "\n  mean end per eighth of the grid:");
            for (int x = 0; x < 8; ++x) {
                double e = 0; int c = 0;
                for (int w = x * nw / 8; w < (x + 1) * nw / 8; ++w) { e += (double)(h[w * 32 + ns - 1] - t0) * 0.01; ++c; }
                fprintf(stderr, " %.1f", e / c);
            }
            double pl = 0;
            for (int w = 0; w < nw; ++w) pl += (double)(h[w * 32 + 1 + 2 * n_layer] - h[w * 32 + 2 * n_layer]) * 0.01;
            fprintf(stderr, "; pooling %.2f\n", pl / nw);
        }
#endif
    };
    if (pool_mode == 0) {
        if (full) { if (H == 256) go(model_kernel<2, false, false>, 0); else go(model_kernel<3, false, false>, 1); }
        else { if (H == 256) go(model_kernel<2, true, false>, 2); else go(model_kernel<3, true, false>, 3); }
    } else {
        if (full) { if (H == 256) go(model_kernel<2, false, true>, 4); else go(model_kernel<3, false, true>, 5); }
        else { if (H == 256) go(model_kernel<2, true, true>, 6); else go(model_kernel<3, true, true>, 7); }
    }
}

}  // namespace bert_hip
