// eval_dev.h -- what the evaluator translation units (eval.hip: the VOC protocol, coco_eval.hip and coco_eval_pooled.hip: the COCO protocol) share: the bits
// of the device error word, the kernels' limits, and on the device the order of fp32
// scores as unsigned integers, the error bits of a frame's counts, the bisection for a class's segment of the sorted records and the
// block-wide scan of the packed (tp, fp) counts.  A change to the error word, the limits or the scan is made here, once.
#pragma once
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_host.h"

// device error word (evaluation.py reports them)
#define EVAL_ERR_UPSTREAM_ABORT 1      // count < 0: an aborted proposal scan upstream
#define EVAL_ERR_GT_OVERFLOW 2         // n_gt > the ground-truth capacity
#define EVAL_ERR_COUNT_RANGE 4         // count > the detection capacity
#define EVAL_ERR_LABEL_RANGE 8         // a label outside 0 .. C-2
#define EVAL_ERR_LEDGER_OVERFLOW 16    // more frames than the image ledger holds (eval_merge.hip)
#define EVAL_ERR_SHARD_TRUNCATED 32    // a merged shard counted more records or ledger rows than its buffer holds (eval_merge.hip)

#define EVAL_MAX_P 2048                // RoI rows per frame: a detection capacity is at most (C-1) * EVAL_MAX_P
#define EVAL_MAX_C 256
#define EVAL_MAX_G 1024
#define EVAL_MAX_T 16
#define EVAL_THREADS 256

typedef unsigned long long u64;

static inline bool eval_supported(int64_t D, int64_t G) { return D >= 1 && D <= (int64_t)(EVAL_MAX_C - 1) * EVAL_MAX_P && G >= 1 && G <= EVAL_MAX_G; }

#ifdef __HIPCC__
// monotone in the float's value; -0 folded onto +0 (Python's sort sees them as equal)
__device__ __forceinline__ uint32_t eval_orderable(float score)
{
    const uint32_t u = __float_as_uint(score == 0.0f ? 0.0f : score);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The error bits of a frame's device counts.  A frame that reports an error (these bits, or a label out of range) is not recorded at
// all: summarize() raises, a partial frame would only hide what was lost.
__device__ __forceinline__ int eval_frame_error(int count, int D, int n_gt, int G)
{
    int e = 0;
    if (count < 0) e |= EVAL_ERR_UPSTREAM_ABORT;
    if (count > D) e |= EVAL_ERR_COUNT_RANGE;
    if (n_gt > G) e |= EVAL_ERR_GT_OVERFLOW;
    return e;
}

// the first index of a[0 .. n), ascending, that holds a value >= v
__device__ __forceinline__ long long eval_lower_bound(const int32_t *__restrict__ a, long long n, int v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One chunk of EVAL_THREADS records of the block-wide inclusive scan of the cumulative (tp, fp), packed into one 64-bit word: tp in the
// low half, fp in the high half (both < 2^32).  `code` is the lane's record at the threshold in hand (FRCNN_EVAL_TP / _FP / _IGNORED;
// 0 past the end of the segment); s_wave holds EVAL_THREADS / 64 words, *s_carry the sum of the chunks before this one (zero, and a
// barrier, before the first).  eval_scan_step returns the lane's inclusive value after the chunk's first barrier.  The caller stores
// what it derives from the value and THEN calls eval_scan_carry, whose two barriers close the chunk: those stores are read by other
// lanes right after the last chunk, so they must lie before a barrier, which is why the step is not one function.
__device__ __forceinline__ u64 eval_scan_step(uint32_t code, u64 *s_wave, const u64 *s_carry)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 v = wave_incl_scan(code == FRCNN_EVAL_TP ? 1ull : (code == FRCNN_EVAL_FP ? 1ull << 32 : 0ull));
    if (lane == 63) s_wave[wv] = v;
    __syncthreads();
    u64 pre = *s_carry;
    for (int w = 0; w < wv; ++w) pre += s_wave[w];
    return v + pre;
}

__device__ __forceinline__ void eval_scan_carry(u64 v, u64 *s_carry)
{
    __syncthreads();
    if (threadIdx.x == EVAL_THREADS - 1) *s_carry = v;
    __syncthreads();
}
#endif
