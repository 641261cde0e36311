// frcnn_dev.h -- the cross-lane and cross-workgroup idioms of the device code, each written and explained ONCE (device only, gfx950).
//   1. agent-scope relaxed accessors        agent_ld / agent_st / agent_add / agent_or
//   2. the last-arriver hand-off            last_arriver / ticket_reset
//   3. LDS-DMA                              dma16_to_lds / barrier_keep_vm[_pinned] / vm_wait<N>
//   4. bf16 conversion                      bf16_rne / bf16_to_f32 / cvt_pk_bf16
//   5. wave reductions, one per association order (a float sum that changes its order changes bits: a call site keeps the one it has)
//   6. the wave scan (the ballot compaction of the input stage is in_compact_slot, input_dev.h)
// Everything here is __device__ __forceinline__ and holds no state; nothing crosses translation units by layout (that is frcnn_layout.h).
// The kernels' instruction streams are pinned (docs/HISTORY.md, "device idioms"): a site was moved onto a function of this header only
// where its kernel came out of the compiler unchanged.  The sites that did not -- a few reductions and scans, five of the six hand-offs --
// keep their own statements, written in this header's vocabulary (agent_*, vm_wait, ticket_reset), and the contracts below hold for
// them all the same.
#pragma once
#include "frcnn_common.h"
#ifdef __HIPCC__

// 1. Agent-scope relaxed accesses: one word, performed at the device's coherence point -- a store is written through this XCD's L2,
// a load or read-modify-write bypasses the CU's L1 and this XCD's L2 -- so it is how workgroups on DIFFERENT XCDs see each other's words
// inside one launch.  Relaxed: it orders nothing else; what a hand-off needs on top is in section 2.  agent_add / agent_or return the OLD value.
// Accesses with another order (eval.hip's acq_rel ticket, nms.hip's acquire fence) are spelled out where they stand.
// FRCNN_RLX_AGENT is the bare argument pair, for the builtin written out at the few sites whose kernel comes out differently behind a
// function: a function's result is known to be defined, a builtin's is not, and the compiler then folds a short-circuit `||` / `&&` or a
// poll loop over it into another instruction order (same values; the three sites say so).
#define FRCNN_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
template <typename T> __device__ __forceinline__ T agent_ld(const T *p) { return __hip_atomic_load(p, FRCNN_RLX_AGENT); }
template <typename T, typename V> __device__ __forceinline__ void agent_st(T *p, V v) { __hip_atomic_store(p, v, FRCNN_RLX_AGENT); }
template <typename T, typename V> __device__ __forceinline__ T agent_add(T *p, V v) { return __hip_atomic_fetch_add(p, v, FRCNN_RLX_AGENT); }
template <typename T, typename V> __device__ __forceinline__ T agent_or(T *p, V v) { return __hip_atomic_fetch_or(p, v, FRCNN_RLX_AGENT); }

// 3a. Hand-placed vector-memory wait.  The compiler counts only the memory operations it emitted itself: a load, store or LDS-DMA issued
// from inline assembly is waited for by exactly these statements.
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 2. The last-arriver hand-off: `total` units of work are spread over workgroups, each writes a partial result to memory and takes
// `add` units off a ticket word; the workgroup whose add completes `total` reduces ALL partials (its own included, read back like the
// others, in a fixed order: the result never depends on who came last) and leaves the ticket zero for the next call.
//   Before the call, every thread's share of the partial is WRITTEN THROUGH: agent_st, or `... sc1` stores from inline assembly.  A plain
//     store may sit dirty in this XCD's L2, where the reducer on another XCD never sees it.
//   last_arriver() then waits for the calling wave's stores to be acknowledged (vm_wait<0>: performed at the coherence point), and the
//     barrier extends that to every wave of the workgroup before thread 0 takes the ticket.  s_flag is an LDS word of the caller's; the
//     second barrier broadcasts the verdict, which is the same in every thread.  Every thread of the workgroup must make the call.
//   The last arriver reads the partials with agent_ld or `sc1` loads ONLY: a plain load may be served from a stale line of its L1 or L2.
//   The ticket is RELAXED on purpose.  With written-through payload and bypassing loads, the acknowledged stores in front of the ticket
//     are the whole hand-off.  An acq_rel ticket (or a release fence in front of it) writes this XCD's dirty lines -- the gradients the
//     kernel has just produced -- back and invalidates its L2 in EVERY workgroup: 20.0 -> 16.6 us for the detection loss at FPN size, and a
//     release fence per workgroup took the conv stage's hand-off from 29 to 130 us per call (docs/HISTORY.md).  eval.hip keeps the fenced form because its payload
//     is plain stores.
//   The ticket must be zero before the first call (the host's job); ticket_reset() by ONE thread of the last arriver re-arms it.
// The sites that write the sequence out (loss.hip, roi_align.hip twice, rpn_conv_f32.hip's Winograd product and weight gradient) differ
// only in where the wait stands (roi_align.hip: inside the asm statement of its stores) and in how the comparison is spelled.
__device__ __forceinline__ bool last_arriver(int *ticket, int add, int total, int &s_flag)
{
    vm_wait<0>();
    __syncthreads();
    if (threadIdx.x == 0) s_flag = (agent_add(ticket, add) + add == total) ? 1 : 0;
    __syncthreads();
    return s_flag != 0;
}
__device__ __forceinline__ void ticket_reset(int *ticket) { agent_st(ticket, 0); }

// 3b. LDS-DMA: 16 bytes per lane, global -> LDS at lds + lane * 16 (lds wave-uniform), no staging registers and no ds_write.  As INLINE
// ASSEMBLY: behind the builtin the compiler tracks the transfer and drains it (vmcnt(0)) in front of the next LDS read that might alias
// it and inside __syncthreads(), so a ring of buffers pays the full round trip every step.  Here the transfer is invisible to the
// compiler: count it with vm_wait<N>() (transfers complete in issue order), then barrier_keep_vm_pinned(), then read.
// m0 holds the LDS destination.  It is a reserved register that the compiler sets right in front of the few instructions that read it
// and does not preserve around an asm statement, so it is written in the SAME statement that uses it (the s_nop is the wait state
// between the two) and nothing is assumed about it afterwards.  The non-temporal variant lives with its one user (rpn_conv_f32.hip).
__device__ __forceinline__ void dma16_to_lds(const float *g, const float *lds)
{
    const unsigned l = (unsigned)(size_t)(const __attribute__((address_space(3))) float *)lds;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(__builtin_amdgcn_readfirstlane(l)), "v"(g) : "memory");
}
// Workgroup barrier that leaves vector-memory operations (an LDS-DMA above all) in flight; __syncthreads() would drain them.
// Two forms, because the instruction streams of both users are pinned (docs/HISTORY.md): barrier_keep_vm_pinned() ends in a compiler
// barrier, so that no memory access the compiler knows of moves across it (roi_align.hip); rpn_conv.hip's kernels were scheduled
// around the bare form and come out differently with the pinned one.  New code takes the pinned form.
__device__ __forceinline__ void barrier_keep_vm()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ void barrier_keep_vm_pinned()
{
    barrier_keep_vm();
    asm volatile("" ::: "memory");
}

// 4. bf16 <-> f32.  Round to nearest even, NaN stays NaN (quiet bit set), as torch's float -> bfloat16.
__device__ __forceinline__ unsigned short bf16_rne(float f)
{
    unsigned u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short b) { return __uint_as_float((unsigned)b << 16); }
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// (lo, hi) -> two bf16 in one dword, same rounding: one v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi)
{
    const bf16x2_t r = __builtin_convertvector((f32x2_t){lo, hi}, bf16x2_t);
    return *(const unsigned *)&r;
}

// 5. Wave reductions over all 64 lanes (every lane active).  Two association orders:
//   xor butterfly  every lane ends with the result, having combined the same pairs;
//   DPP chain      row shifts and row broadcasts on the VALU (no LDS crossbar): result in lane 63 only (_dpp), or read from it (_dpp_all);
// (The two shuffle-down trees, photometric.hip and rpn_conv_f32.hip, stay where they are: see the note at the top.)
template <typename T, typename Op> __device__ __forceinline__ T wave_reduce_xor(T v, Op op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum_xor(T v) { return wave_reduce_xor(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ double wave_sum_xor(double v) { return wave_reduce_xor(v, [](double a, double b) { return __dadd_rn(a, b); }); }
__device__ __forceinline__ float wave_max_xor(float v) { return wave_reduce_xor(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ unsigned long long wave_max_xor(unsigned long long k)          // 6 steps on both halves
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, o);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), o);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        k = other > k ? other : k;
    }
    return k;
}
// `identity` is what a lane without a source (row_shr past the row's start) combines with.
template <typename Op> __device__ __forceinline__ float wave_reduce_dpp(float v, float identity, Op op)
{
#define FRCNN_DPP_STEP(ctrl, rmask)                                                                                                \
    v = op(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v), ctrl, rmask, 0xf, false)))
    FRCNN_DPP_STEP(0x111, 0xf);    // row_shr:1
    FRCNN_DPP_STEP(0x112, 0xf);    // row_shr:2
    FRCNN_DPP_STEP(0x114, 0xf);    // row_shr:4
    FRCNN_DPP_STEP(0x118, 0xf);    // row_shr:8   -> lane 15 of every row holds the row's result
    FRCNN_DPP_STEP(0x142, 0xa);    // row_bcast:15 into rows 1 and 3
    FRCNN_DPP_STEP(0x143, 0xc);    // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's result
#undef FRCNN_DPP_STEP
    return v;
}
// the 64-bit maximum by the same chain, both halves moved together: lane 63 ends with the wave's result; a lane without a source combines with 0
__device__ __forceinline__ unsigned long long wave_max_dpp(unsigned long long k)
{
#define FRCNN_DPP_STEP64(ctrl, rmask)                                                                                              \
    do {                                                                                                                           \
        const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, ctrl, rmask, 0xf, false);                   \
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), ctrl, rmask, 0xf, false);           \
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;                                                      \
        k = other > k ? other : k;                                                                                                 \
    } while (0)
    FRCNN_DPP_STEP64(0x111, 0xf);  // row_shr:1
    FRCNN_DPP_STEP64(0x112, 0xf);  // row_shr:2
    FRCNN_DPP_STEP64(0x114, 0xf);  // row_shr:4
    FRCNN_DPP_STEP64(0x118, 0xf);  // row_shr:8   -> lane 15 of every row holds the row's result
    FRCNN_DPP_STEP64(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    FRCNN_DPP_STEP64(0x143, 0xc);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's result
#undef FRCNN_DPP_STEP64
    return k;
}
__device__ __forceinline__ float wave_lane63(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)); }
__device__ __forceinline__ float wave_sum_dpp(float v) { return wave_reduce_dpp(v, 0.0f, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ float wave_max_dpp(float v) { return wave_reduce_dpp(v, -__builtin_inff(), [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ float wave_max_dpp_all(float v) { return wave_lane63(wave_max_dpp(v)); }

// 6. wave_incl_scan: inclusive scan over the wave's lanes in lane order.  The block-wide scans built on it (targets.hip, topk.hip,
// eval_merge.hip, eval_dev.h, nms.hip) differ in how they add up the earlier waves' totals and keep those few lines to themselves;
// so do three scans whose kernels change behind the call (targets.hip's digit search, roi_align.hip's plan, coco_eval.hip's running maximum).
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
#endif  // __HIPCC__
