// device.h — the device-side building blocks that more than one kernel file uses (gfx950): vector types, address-space casts,
// compile-time loops, the in-kernel timeline stamps of the tuning builds, hand-issued LDS reads and the waits around them, the
// tile swizzle, lane-crossing reductions, the int8 row rule, the softmax numerators, packed GELU, LayerNorm statistics, q4 block expansion and the
// per-lane LayerNorm of the fused kernels.  Host code includes kernels.h only.
//
// The kernels that stream weight tiles through LDS rings (gemm256.hip, layer_tail.hip, qkv_attention2.hip, skinny.hip): 128-row
// x 64-half tiles travel HBM/L2 -> LDS by global_load_lds_dwordx4 several tiles ahead of their use and are retired with a
// counted s_waitcnt vmcnt(N) plus one s_barrier per tile; the 16-byte chunk of every row is XOR-swizzled on the SOURCE side
// (LDS-DMA writes lane-linearly) and un-swizzled by the ds_read_b128 reads.
#pragma once
#include "kernels.h"

#include <cstdio>
#include <type_traits>
#include <utility>

namespace bert_hip {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x16 __attribute__((ext_vector_type(16)));

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N-1>{})
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

// address-space casts for the LDS-DMA builtin, and typed LDS pointers (plain loads through a generic pointer become flat loads)
#define AS_GLOBAL(p) ((const __attribute__((address_space(1))) void *)(p))
#define AS_LDS(p) ((__attribute__((address_space(3))) void *)(p))
template <class T>
using lds_cptr = const __attribute__((address_space(3))) T *;


// Tuning aid, compiled in only with -DBERT_HIP_TIMELINE: thread 0 of every workgroup stamps the shader clock
// (TL_STAMP) at the top of each interval; the launcher (TL_DUMP) prints the deltas of a few workgroups of its
// 21st large launch to stderr.  Not part of the product build.
#ifdef BERT_HIP_TIMELINE
static __device__ unsigned long long g_timeline[1024 * 256];
#define TL_STAMP(i) do { const int tl_i = (i); if (threadIdx.x == 0 && tl_i < 256) g_timeline[(blockIdx.x & 1023) * 256 + tl_i] = __builtin_readcyclecounter(); } while (0)
#define TL_STAMP_AT(sel, i) do { const int tl_i = (i); if ((sel) && tl_i < 256) g_timeline[(blockIdx.x & 1023) * 256 + tl_i] = __builtin_readcyclecounter(); } while (0)
// the constant 100 MHz counter next to the shader clock: (cycles between two stamps) / (real time between them) = the clock
#define TL_REALTIME_AT(sel, i) do { const int tl_i = (i); if ((sel) && tl_i < 256) g_timeline[(blockIdx.x & 1023) * 256 + tl_i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define TL_DUMP(cond, nstamps) do {                                                                          \
    static int tl_shots = 0;                                                                                  \
    if ((cond) && tl_shots++ == 20) {                                                                         \
        (void)hipDeviceSynchronize();                                                                         \
        static unsigned long long tl_h[1024 * 256];                                                           \
        (void)hipMemcpyFromSymbol(tl_h, HIP_SYMBOL(g_timeline), sizeof(tl_h));                                \
        const int tl_n = (nstamps) < 256 ? (nstamps) : 256;                                                   \
        for (int b : {0, 1, 100, 255}) {                                                                      \
            fprintf(stderr, "timeline wg %3d:", b);                                                           \
            for (int i = 1; i < tl_n; ++i) fprintf(stderr, " %llu", tl_h[b * 256 + i] - tl_h[b * 256 + i - 1]); \
            fprintf(stderr, "  total %llu\n", tl_h[b * 256 + tl_n - 1] - tl_h[b * 256]);                      \
        }                                                                                                     \
    }                                                                                                         \
} while (0)
// raw stamps relative to stamp 0 (kernels whose waves stamp disjoint index ranges)
#define TL_DUMP_RAW(cond, nstamps) do {                                                                      \
    static int tl_shots = 0;                                                                                  \
    if ((cond) && tl_shots++ == 20) {                                                                         \
        (void)hipDeviceSynchronize();                                                                         \
        static unsigned long long tl_h[1024 * 256];                                                           \
        (void)hipMemcpyFromSymbol(tl_h, HIP_SYMBOL(g_timeline), sizeof(tl_h));                                \
        for (int b : {0, 100}) {                                                                              \
            fprintf(stderr, "rawtimeline wg %3d:", b);                                                        \
            for (int i = 0; i < (nstamps); ++i)                                                               \
                fprintf(stderr, " %lld", tl_h[b * 256 + i] ? (long long)(tl_h[b * 256 + i] - tl_h[b * 256]) : -1LL); \
            fprintf(stderr, "\n");                                                                            \
        }                                                                                                     \
    }                                                                                                         \
} while (0)
#else
#define TL_DUMP_RAW(cond, nstamps) do { } while (0)
#define TL_REALTIME_AT(sel, i) do { } while (0)
#define TL_STAMP(i) do { } while (0)
#define TL_STAMP_AT(sel, i) do { } while (0)
#define TL_DUMP(cond, nstamps) do { } while (0)
#endif

// ---- hand-issued LDS reads.  The compiler's wait insertion retires LDS reads with lgkmcnt(0) only; a wave that
// has a matrix pipe to itself must keep reads in flight under its MFMAs, so the self-pipelined kernels issue
// their fragment reads as asm and retire them with partial counts (LDS operations complete in order).  Rules:
// every such read is covered by an explicit wait that names the destination registers ("+v"), and no
// compiler-generated LDS access may sit between a group of reads and its partial wait ("memory" clobbers keep them out).
// MEMORY: whether the read itself carries that clobber.  true: the read is a compiler barrier for memory accesses of its own
// (layer_tail.hip, whose intervals also hold compiler-generated LDS and global accesses).  false: only the waits are
// (gemm256.hip, qkv_attention2.hip), and the compiler schedules the code around the reads more freely.  Keep a kernel's form:
// switching it changes that kernel's machine code (gemm256's scalar address code, for one).
__device__ __forceinline__ unsigned lds_addr(const void *p) {
    return (unsigned)(size_t)(__attribute__((address_space(3))) const char *)p;
}
template <bool MEMORY, int OFF, class V = f16x8>
__device__ __forceinline__ V lds_read_b128(unsigned addr) {
    static_assert(sizeof(V) == 16, "ds_read_b128 reads 16 bytes");
    static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
    V v;
    if constexpr (MEMORY) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    else asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
// a hand-read (or untracked) register handed to its users, behind the wait that retired the read
template <class V>
__device__ __forceinline__ void landed(V &v) { asm volatile("" : "+v"(v)); }
// workgroup barrier behind this wave's DMA pieces (all but the newest VM have landed) and all of its LDS reads and writes
template <int VM>
__device__ __forceinline__ void dma_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" : : "n"(VM) : "memory");
}

// byte offset of 16-byte chunk `chunk` of row `row` in a [rows x 64 halfs] tile: the chunk swizzle of conflict-free ds_read_b128
__device__ __forceinline__ int off64(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// An f32 value the compiler must materialise: (_Float16)rounded_f32(a * b) is an f32 multiply followed by a conversion,
// never the fused v_fma_mixlo_f16 (ONE rounding, to f16).  Which of the two forms the compiler picks for (_Float16)(a * b)
// depends on the surrounding code, and kernels that must agree bit for bit (attention.hip, qkv_attention*.hip) would
// differ in one result of ~20 000.
__device__ __forceinline__ float rounded_f32(float v) {
    asm("" : "+v"(v));
    return v;
}

// ---- lane-crossing reductions without the LDS.  __shfl_xor is a ds_bpermute_b32: an LDS round trip (and an lgkmcnt wait) per step.
// The same PAIRS meet here — so sums and maxima keep their bits — through v_permlane32_swap (lane ^ 32: the two halves of the wave
// trade places), ds_swizzle (lane ^ 16 / 8 / 4: no address register, no LDS access) and DPP quad_perm on the add itself (lane ^ 2 / 1).
// tools/ubench/wave_sum.hip checks the six-step sum against the __shfl_xor butterfly bit for bit.
// xor32_pair: a = this lane's value, b = lane ^ 32's in the low half of the wave and the other way round in the high half — fine for
// commutative uses (a + b, max(a, b)).  By hand: this compiler's __builtin_amdgcn_permlane32_swap returns its first result twice; the
// instruction needs two registers (with one as both operands it copies the low half up and loses the high one); the wait states
// between a VALU write and a lane-crossing read are ours inside an asm.
__device__ __forceinline__ void xor32_pair(float &a, float &b) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
// A 32x32 MFMA RESULT fragment (lane (l31, hi) holds columns 16 q + 4 hi + {0..3} | 16 q + 8 + 4 hi + {0..3} of row l31, rounded to f16)
// as the OPERAND fragment of k-step q (lane (l31, hi): k = 16 q + 8 hi + {0..7} of the same row): lanes 0..31 give their upper half for
// the lower half of lanes 32..63 — v_permlane32_swap vdst, src exchanges lanes 32..63 of vdst with lanes 0..31 of src, one dword at a time
// — and every element already sits in its place.
__device__ __forceinline__ f16x8 result_to_operand_fragment(const f16x8 &v) {
    const u32x4 d = __builtin_bit_cast(u32x4, v);
    uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3\n\ts_nop 1" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3));
    return __builtin_bit_cast(f16x8, u32x4{d0, d1, d2, d3});
}
// model_kernel.hip's window -> tail edge: where the last two heads' context fragments wait in LDS for the tail's waves (block b: 4 KiB at
// + 4096 b) — behind the exchange area of the heads before them (nq KiB per block, from 0) and inside what both phases leave alone at the
// edge: the tail's idle third ring slot / GELU area from 80 KiB on, the window phase's dead ring or dead Q/K/V copy
constexpr int ctx_edge_offset(int nq) { return nq * 4096 > 80 * 1024 ? nq * 4096 : 80 * 1024; }
__device__ __forceinline__ float xor32_sum(float v) { float a = v, b = v; xor32_pair(a, b); return a + b; }
__device__ __forceinline__ float xor32_max(float v) { float a = v, b = v; xor32_pair(a, b); return __builtin_fmaxf(a, b); }
// v + (lane ^ 32) + ... + (lane ^ 1), the pairs and the order of the __shfl_xor butterfly from 32 down to 1
__device__ __forceinline__ float wave_sum_f32(float v) {
    v = xor32_sum(v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (16 << 10) | 0x1F));
    v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (8 << 10) | 0x1F));
    v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (4 << 10) | 0x1F));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    return v;
}

// The int8 row rule of the embedding index (search.hip index_quantize_kernel) and the token index (token_index.hip
// token_i8_quantize_kernel), the whole wave on one row: x[0 .. dim) (f32, or f16 converted exactly) -> scale = amax / 127 and codes
// out[0 .. dpad) = clamp(rint(x_i / scale), -127, 127), zero from dim on.  All codes 0 where the scale is 0; scale NaN and codes 0 where an
// element is NaN or +-inf.  The finite test and the maximum of |x_i| across the wave (a maximum is exact in any lane order), then four
// codes per lane and 32-bit store.  dpad is a multiple of 32; the division is IEEE (correctly rounded), rint rounds to nearest even.
template <class T>
__device__ __forceinline__ void quantize_row_i8(const T *__restrict__ x, int dim, int dpad, int8_t *__restrict__ out, float *__restrict__ scale_out,
                                                int lane) {
    float amax = 0.f;
    int bad = 0;
    for (int c = lane; c < dim; c += 64) {
        const float v = (float)x[c];
        bad |= !__builtin_isfinite(v);                         // (fmaxf drops a NaN: tested on its own)
        amax = fmaxf(amax, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    bad = __any(bad);
    const float scale = bad ? __builtin_nanf("") : amax / 127.0f;
    const bool zero = bad || scale == 0.f;
    if (lane == 0) *scale_out = scale;
    for (int c = 4 * lane; c < dpad; c += 256) {
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = c + j < dim ? (float)x[c + j] : 0.f;
            const float q = zero ? 0.f : fminf(fmaxf(__builtin_rintf(v / scale), -127.f), 127.f);
            packed |= (uint32_t)(uint8_t)(int8_t)(int)q << (8 * j);
        }
        *(uint32_t *)(out + c) = packed;
    }
}

// Softmax numerators of EIGHT scores of one query (registers 8 st .. 8 st + 7 of an S^T tile = the B fragment of one P·V MFMA
// step) — ONE function for all attention bodies (attention.hip, qkv_attention2.hip and with it model_kernel.hip): equal bits
// across the routes.  Two forms:
//   BERT_HIP_EXP16 = 0 (default): p = exp2(fma(s, sc, -m)) in f32 (v_fma_f32, v_exp_f32), the row sum an f32 add, P rounded to
//     f16 for the V mat-mul (v_cvt_pk_f16_f32) — rounds 1-4's arithmetic.
//   BERT_HIP_EXP16 = 1: the reference's own precision — ggml's soft_max rounds (s - max) to fp16 and reads an fp16 table of exp
//     (reference bert.cpp:845 -> ggml_soft_max; oracle/bert_oracle.cpp:544): the argument one fma rounded ONCE to f16
//     (v_fma_mixlo / mixhi_f16 write the two halves of a register), v_exp_f16 on each half (the high one through SDWA with the
//     low half preserved), the pair IS the MFMA operand, the row sum f32 through v_dot2c_f32_f16 with (1, 1).  21 instructions
//     per 8 scores against 28 — and SLOWER on this chip (round 5, tools/ubench/valu_cost.hip, profiles/r5_valu_cost.txt):
//     v_fma_mix* issue at the transcendental rate (7.9 cycles per instance and wave beside MFMAs, 2 waves per SIMD, against 2.5
//     for v_fma_f32) and v_dot2c shares the matrix pipe (8.6 against 1.9 for v_add_f32): 40 cycles per score pair against 27.
//     Measured end to end: headline 327.0 k against 330.5 k sentences/s on one box, attention at 512 tokens 9.28 against 8.68 ms
//     per 12 launches.  Parity-green (395 tests) and kept as a build option; not the default.
// The trailing s_nop of the fp16 form: gfx940+ needs one wait state between an instruction that writes half a register (SDWA
// dst_sel) and a reader of that register, and the compiler's hazard pass does not look into an asm block.
#ifndef BERT_HIP_EXP16
#define BERT_HIP_EXP16 0
#endif
// the three steps of softmax_p8 on four score PAIRS, separately callable so that a kernel can put MFMAs between them
// (attention.hip's software-pipelined chunk loop): arguments (8 VALU), exponentials (8 VALU + the wait state), row sum (4 dot2);
// softmax_pack: the B fragment of the P·V MFMA step (the exponentials themselves in the fp16 form).
// -DBERT_HIP_EXP16=0 (tuning builds): the f32 form of rounds 1-4 — fma, v_exp_f32, add, v_cvt_pk_f16_f32.
#if BERT_HIP_EXP16
typedef u32x4 sm_arg_t;
typedef u32x4 sm_exp_t;
__device__ __forceinline__ sm_arg_t softmax_args4(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7, float sc, float m) {
    uint32_t a0, a1, a2, a3;            // (scalar outputs: asm outputs that are elements of a vector come out wrong)
    asm("v_fma_mixlo_f16 %0, %4, %12, -%13\n\t"
        "v_fma_mixlo_f16 %1, %6, %12, -%13\n\t"
        "v_fma_mixlo_f16 %2, %8, %12, -%13\n\t"
        "v_fma_mixlo_f16 %3, %10, %12, -%13\n\t"
        "v_fma_mixhi_f16 %0, %5, %12, -%13\n\t"
        "v_fma_mixhi_f16 %1, %7, %12, -%13\n\t"
        "v_fma_mixhi_f16 %2, %9, %12, -%13\n\t"
        "v_fma_mixhi_f16 %3, %11, %12, -%13"
        : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3)
        : "v"(s0), "v"(s1), "v"(s2), "v"(s3), "v"(s4), "v"(s5), "v"(s6), "v"(s7), "s"(sc), "v"(m));
    return u32x4{a0, a1, a2, a3};
}
__device__ __forceinline__ sm_exp_t softmax_exp4(sm_arg_t a) {
    uint32_t p0, p1, p2, p3;
    asm("v_exp_f16_e32 %0, %4\n\t"
        "v_exp_f16_e32 %1, %5\n\t"
        "v_exp_f16_e32 %2, %6\n\t"
        "v_exp_f16_e32 %3, %7\n\t"
        "v_exp_f16_sdwa %0, %4 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"
        "v_exp_f16_sdwa %1, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"
        "v_exp_f16_sdwa %2, %6 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"
        "v_exp_f16_sdwa %3, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"
        "s_nop 0"
        : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
        : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
    return u32x4{p0, p1, p2, p3};
}
__device__ __forceinline__ void softmax_sum4(sm_exp_t p, float &psum) {
    const f16x2 one = {(_Float16)1.0f, (_Float16)1.0f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t pe = p[e];       // (a scalar copy: __builtin_bit_cast applied to a vector ELEMENT reads element 0 whatever e is)
        psum = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, pe), one, psum, false);
    }
}
__device__ __forceinline__ f16x8 softmax_pack(sm_exp_t p) { return __builtin_bit_cast(f16x8, p); }
#else
typedef f32x8 sm_arg_t;
typedef f32x8 sm_exp_t;
__device__ __forceinline__ sm_arg_t softmax_args4(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7, float sc, float m) {
    const float s[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
    f32x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = __builtin_fmaf(s[e], sc, -m);
    return a;
}
__device__ __forceinline__ sm_exp_t softmax_exp4(sm_arg_t a) {
    f32x8 p;
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = __builtin_amdgcn_exp2f(a[e]);
    return p;
}
__device__ __forceinline__ void softmax_sum4(sm_exp_t p, float &psum) {
#pragma unroll
    for (int e = 0; e < 8; ++e) psum += p[e];
}
__device__ __forceinline__ f16x8 softmax_pack(sm_exp_t p) {
    f16x8 pf;
#pragma unroll
    for (int e = 0; e < 8; ++e) pf[e] = (_Float16)p[e];
    return pf;
}
#endif
__device__ __forceinline__ f16x8 softmax_p8(float s0, float s1, float s2, float s3, float s4, float s5, float s6, float s7, float sc,
                                            float m, float &psum) {
    const sm_exp_t p = softmax_exp4(softmax_args4(s0, s1, s2, s3, s4, s5, s6, s7, sc, m));
    softmax_sum4(p, psum);
    return softmax_pack(p);
}
// tanh-form GELU of two values, packed f16: x / (1 + 2^(x (c1 + c2 x^2)))
__device__ __forceinline__ f16x2 gelu_pk16h(f16x2 xh) {
    const float c1 = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f;
    const f16x2 C1 = {(_Float16)c1, (_Float16)c1}, C2 = {(_Float16)(c1 * 0.044715f), (_Float16)(c1 * 0.044715f)};
    const f16x2 one = {(_Float16)1.0f, (_Float16)1.0f};
    const f16x2 t = (xh * xh * C2 + C1) * xh;
    const f16x2 e = {(_Float16)__builtin_exp2f16(t[0]), (_Float16)__builtin_exp2f16(t[1])};
    const f16x2 d = e + one;
    const f16x2 r = {(_Float16)__builtin_amdgcn_rcph(d[0]), (_Float16)__builtin_amdgcn_rcph(d[1])};
    return xh * r;
}
__device__ __forceinline__ f16x2 gelu_pk16(float a0, float a1) { return gelu_pk16h(f16x2{(_Float16)a0, (_Float16)a1}); }

// LayerNorm statistics (sum, sum of squares over H values) -> (1 / std, -mean / std), eps 1e-5 (ggml's).  Every product and
// sum is spelled out: with -ffp-contract=fast the compiler picks which a * b + c it fuses by the surrounding code, and kernels
// that must agree bit for bit (layer_tail.hip and its feature-split mirror skinny.hip) share this function instead.
// 1 / sqrt = v_rsq_f32 + one Newton step (1 ulp).
__device__ __forceinline__ void layernorm_scale(float s1, float s2, float inv_h, float &rstd, float &nmr) {
    const float mean = s1 * inv_h, ex2 = s2 * inv_h;
    const float t = fmaxf(__builtin_fmaf(-mean, mean, ex2), 0.f) + 1e-5f;
    const float r = __builtin_amdgcn_rsqf(t);
    rstd = r * __builtin_fmaf(-0.5f * t, r * r, 1.5f);
    nmr = -mean * rstd;
}

// ---- q4 blocks -> f16 tiles.  A thread expands one block of 32 weights (16 bytes of nibbles: byte j = element j | element
// j + 16 << 4; f16 d, or f16 {d, m}) into four 16-byte chunks of its row: v_perm_b32 builds (1024 + q) half pairs, packed f16
// math applies (q - 8) d or q d + m — the values the f16 image holds (weights.cpp row_to_f16).
struct RawBlock { uint4 q; unsigned sc; };
template <int WT>
__device__ __forceinline__ RawBlock q4_load_block(const uint4 *qs, const void *sc, size_t index) {
    RawBlock r;
    r.q = qs[index];
    r.sc = WT == GW_Q4_0 ? (unsigned)((const unsigned short *)sc)[index] : ((const unsigned *)sc)[index];
    return r;
}
// the scale decode and the constants of one block's expansion
template <int WT>
struct Q4Expansion {
    f16x2 d2, m2, off;
    unsigned magic, sel01, sel23;
    __device__ __forceinline__ explicit Q4Expansion(unsigned sc) {
        if (WT == GW_Q4_0) {
            const _Float16 d = __builtin_bit_cast(_Float16, (unsigned short)(sc & 0xffffu));
            d2 = (f16x2){d, d};
            m2 = (f16x2){(_Float16)0, (_Float16)0};
        } else {
            const f16x2 dm = __builtin_bit_cast(f16x2, sc);
            d2 = (f16x2){dm[0], dm[0]};
            m2 = (f16x2){dm[1], dm[1]};
        }
        // The constants are made HERE, per call, behind opaque moves (gfx9 VOP3 takes no literals and one scalar operand: the
        // byte source of v_perm_b32 has to sit in a vector register): hoisted out of the caller's loop they cost three registers
        // for the whole kernel — or, in kernels that have none to spare, a scratch reload per use.
        unsigned offb;
        asm volatile("v_mov_b32 %0, 0x64646464" : "=v"(magic));
        asm volatile("s_mov_b32 %0, 0x04010400" : "=s"(sel01));
        asm volatile("s_mov_b32 %0, 0x04030402" : "=s"(sel23));
        if (WT == GW_Q4_0) asm volatile("s_mov_b32 %0, 0x64086408" : "=s"(offb));      // 1032, 1032
        else asm volatile("s_mov_b32 %0, 0x64006400" : "=s"(offb));                    // 1024, 1024
        off = __builtin_bit_cast(f16x2, offb);
    }
    // the four weights of the low (high) nibbles of `word`: two f16 pairs.  q4_1: q d + m rounded once (weights.cpp row_to_f16).
    // Q_FIRST: the operand order of that fma — the same value either way, but each caller's machine code keeps its own order.
    template <bool Q_FIRST>
    __device__ __forceinline__ void four(unsigned word, bool high, unsigned &o0, unsigned &o1) const {
        const unsigned n4 = (high ? (word >> 4) : word) & 0x0f0f0f0fu;
        f16x2 v0 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, n4, sel01)) - off;
        f16x2 v1 = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(magic, n4, sel23)) - off;
        if (WT == GW_Q4_0) { v0 = v0 * d2; v1 = v1 * d2; }
        else if (Q_FIRST) { v0 = __builtin_elementwise_fma(v0, d2, m2); v1 = __builtin_elementwise_fma(v1, d2, m2); }
        else { v0 = __builtin_elementwise_fma(d2, v0, m2); v1 = __builtin_elementwise_fma(d2, v1, m2); }
        o0 = __builtin_bit_cast(unsigned, v0);
        o1 = __builtin_bit_cast(unsigned, v1);
    }
};
// The whole block: chunk_ptr(c) is where chunk c goes.  PERM: the k order inside every group of 16 is [0-3, 8-11, 4-7, 12-15]
// (GemmWeight::w16p), plain otherwise.
template <int WT, bool PERM, class ChunkPtr>
__device__ __forceinline__ void q4_expand_block(const RawBlock &r, ChunkPtr chunk_ptr) {
    const unsigned w[4] = {r.q.x, r.q.y, r.q.z, r.q.w};
    const Q4Expansion<WT> x(r.sc);
#pragma unroll
    for (int h = 0; h < 2; ++h)                               // elements 0..15 (low nibbles) / 16..31 (high nibbles)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            // chunk 2 h + pr: plain = elements 8 pr .. + 8 of the half (words 2 pr, 2 pr + 1); PERM = {4 pr .., 8 + 4 pr ..} (words pr, pr + 2)
            uint4 out;
            x.template four<false>(w[PERM ? pr : 2 * pr], h, out.x, out.y);
            x.template four<false>(w[PERM ? pr + 2 : 2 * pr + 1], h, out.z, out.w);
            *(uint4 *)chunk_ptr(2 * h + pr) = out;
        }
}
// One 16-byte chunk (eight weights, plain k order: elements 8 c .. 8 c + 7 of the block): for kernels that spread a block's
// expansion over several issue gaps (gemm256.hip).
template <int WT>
__device__ __forceinline__ uint4 q4_expand_chunk(const RawBlock &r, int c) {
    const Q4Expansion<WT> x(r.sc);
    const bool high = c >= 2;
    const unsigned w0 = (c & 1) ? r.q.z : r.q.x, w1 = (c & 1) ? r.q.w : r.q.y;
    uint4 out;
    x.template four<true>(w0, high, out.x, out.y);
    x.template four<true>(w1, high, out.z, out.w);
    return out;
}

// LayerNorm of one token's row from f32 values, the way layer_tail.hip's lanes and wave pairs do it (the latency route:
// skinny.hip, and the per-head form of qkv_attention2.hip): lane = (token l31, half hi) holds the
// 4-feature runs (n, g) = features 32 n + 8 g + 4 hi .. + 3 of its token (H / 2 values, loaded 16 bytes at a time).
// PAIR (LayerNorm 1): the statistics are the sum of two half-row sums (features with (f & 127) < 64: layer_tail's U wave;
// the rest: its D wave), each summed block by block, register by register, then across the lane halves; !PAIR (LayerNorm
// 2): one sum over all blocks (the D wave owns whole rows).  Result: the normalised runs, f16.
template <bool PAIR, int NT, class Run, class Landed>
__device__ __forceinline__ void layernorm_runs_of(Run x, Landed landed, const float *gamma, const float *beta, int hi, f16x4 (&y)[4 * NT][4]) {
    constexpr int H = 128 * NT;
    // the parameter reads run AHEAD blocks (eight 16-byte loads each) in front of their use — spelled out: the compiler's own
    // order waits for every pair of loads in turn (48 L2 round trips)
    constexpr int AHEAD = 2;
    f32x4 gv[AHEAD + 1][4], bv[AHEAD + 1][4];
    auto request = [&](int n) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            gv[n % (AHEAD + 1)][g] = *(const f32x4 *)(gamma + 32 * n + 8 * g + 4 * hi);
            bv[n % (AHEAD + 1)][g] = *(const f32x4 *)(beta + 32 * n + 8 * g + 4 * hi);
        }
    };
#pragma unroll
    for (int n = 0; n < AHEAD; ++n) request(n);
    landed();                          // (runs that arrive by LDS-DMA: the wait for them, behind the first parameter requests)
    float s1 = 0.f, s2 = 0.f;
    auto add_block = [&](float &a1, float &a2, int n) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = x(n, g);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a1 += v[e]; a2 = __builtin_fmaf(v[e], v[e], a2); }
        }
    };
    if constexpr (PAIR) {
        float t1[2] = {0.f, 0.f}, t2[2] = {0.f, 0.f};
#pragma unroll
        for (int role = 0; role < 2; ++role)
#pragma unroll
            for (int b = 0; b < 2 * NT; ++b) add_block(t1[role], t2[role], (b >> 1) * 4 + role * 2 + (b & 1));
#pragma unroll
        for (int role = 0; role < 2; ++role) { t1[role] += __shfl_xor(t1[role], 32); t2[role] += __shfl_xor(t2[role], 32); }
        s1 = t1[0] + t1[1]; s2 = t2[0] + t2[1];
    } else {
#pragma unroll
        for (int n = 0; n < 4 * NT; ++n) add_block(s1, s2, n);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
    }
    float rstd, nmr;
    layernorm_scale(s1, s2, 1.0f / H, rstd, nmr);
    asm volatile("" ::: "memory");     // (runs that come from LDS are read again instead of being kept: registers for the loads in flight)
#pragma unroll
    for (int n = 0; n < 4 * NT; ++n) {
        if (n + AHEAD < 4 * NT) request(n + AHEAD);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = x(n, g), gq = gv[n % (AHEAD + 1)][g], bq = bv[n % (AHEAD + 1)][g];
            // (f32 results, THEN f16: fused into v_fma_mixlo_f16 — one rounding — the compiler's choice depends on the kernel around
            // it.  One opaque hand-over per run of four, so that the f32 math itself still packs into v_pk_fma_f32.)
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(v[e], gq[e] * rstd, __builtin_fmaf(gq[e], nmr, bq[e]));
            asm("" : "+v"(r));
#pragma unroll
            for (int e = 0; e < 4; ++e) y[n][g][e] = (_Float16)r[e];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the runs from memory: all of the row in registers first
template <bool PAIR, int NT>
__device__ __forceinline__ void layernorm_runs(const float *row, const float *gamma, const float *beta, int hi, f16x4 (&y)[4 * NT][4]) {
    f32x4 x[4 * NT][4];
#pragma unroll
    for (int n = 0; n < 4 * NT; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) x[n][g] = *(const f32x4 *)(row + 32 * n + 8 * g + 4 * hi);
    layernorm_runs_of<PAIR, NT>([&](int n, int g) __attribute__((always_inline)) { return x[n][g]; }, [] {}, gamma, beta, hi, y);
}

}  // namespace bert_hip
