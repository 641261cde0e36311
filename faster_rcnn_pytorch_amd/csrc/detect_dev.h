// detect_dev.h -- what the fused detection post-process (detect.hip) and the merge of detection sets (detect_merge.hip) share: the
// orderable form of a score and the in-LDS bitonic sort of 64-bit keys, so that both order their candidates with the same instructions.
#pragma once
#include "frcnn_common.h"

#ifdef __HIPCC__
typedef unsigned long long det_u64;

// score descending as an ascending 32-bit word; the scores that reach it passed `score > thr`, hence are not NaN.  -0 is folded onto +0:
// the reference's sort sees them as equal.
__device__ __forceinline__ uint32_t det_score_word(float score)
{
    uint32_t u = __float_as_uint(score == 0.0f ? 0.0f : score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);               // monotone in the float's value
    return ~u;
}

// (score descending, low word ascending) as one ascending 64-bit key
__device__ __forceinline__ det_u64 det_key(float score, uint32_t low) { return ((det_u64)det_score_word(score) << 32) | low; }

// bitonic sort of M keys (a power of two, the tail padded with ~0) in LDS, ascending, by the whole workgroup of THREADS threads; ends
// with a barrier
template <int THREADS> __device__ __forceinline__ void det_bitonic_sort(det_u64 *s_key, int M, int tid)
{
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (M >> 1); t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i + j;
                const det_u64 a = s_key[i], b = s_key[l];
                if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
            }
            __syncthreads();
        }
}
#endif  // __HIPCC__
