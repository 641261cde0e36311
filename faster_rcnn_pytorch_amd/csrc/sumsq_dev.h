// sumsq_dev.h -- the chunk body of the sum-of-squares contract written down in include/frcnn_hip.h (frcnn_grad_norm: element, chunk,
// wave, block), once, for grad_norm.hip (the global gradient norm) and telemetry.hip (per-tensor statistics of g, p and m): both run
// THIS code, so a chunk's partial is the same bits in both workspaces.
//
//   sumsq_chunk_wave<MAX>   the calling thread's share of a chunk of n <= SGD_CHUNK elements at x -- thread t = (i / 4) % SGD_THREADS owns
//                           element i, one binary64 accumulator per i % 4, squares in increasing i, a = (a0 + a1) + (a2 + a3) -- then the
//                           xor butterfly of its wave: every lane returns the wave's sum, the wave's count of non-finite elements and,
//                           with MAX, the wave's max|x| (the `>` comparison from +0: a NaN never wins, an inf does; order-free).
//   sumsq_block4            ((w0 + w1) + w2) + w3, the four waves in wave order.
//
// The square of a binary32 is exact in binary64, so fma(d, d, acc) and acc + d * d are the same number and contraction cannot change a
// bit; every other addition is written out (__dadd_rn).  Loads: 16-byte when x itself is 16-byte aligned, dword loads otherwise, with the
// same element-to-thread assignment.  Default cache policy.  x == nullptr with n == 0 is legal (nothing is loaded).
#pragma once
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "sgd_dev.h"

static_assert(SGD_THREADS == 4 * WAVE, "a chunk's workgroup adds four waves in order");

template <bool MAX>
__device__ __forceinline__ void sumsq_take(float x, double &acc, int &bad, float &mx)
{
    const double d = (double)x;
    acc = __fma_rn(d, d, acc);
    bad += ((__float_as_uint(x) >> 23) & 0xffu) == 0xffu;
    if (MAX) {
        const float a = fabsf(x);
        if (a > mx) mx = a;
    }
}

template <bool MAX>
__device__ __forceinline__ double sumsq_chunk_wave(const float *__restrict__ x, int n, int tid, int &bad_out, float &max_out)
{
    const int n4 = n >> 2;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    float mx = 0.0f;
    if (((uintptr_t)x & 15) == 0) {
        const sgd_f4 *x4 = (const sgd_f4 *)x;
        for (int base = 0; base < n4; base += 4 * SGD_THREADS) {
            sgd_f4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * SGD_THREADS + tid;
                if (i < n4) v[k] = x4[i];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * SGD_THREADS + tid;
                if (i < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) sumsq_take<MAX>(v[k][e], a[e], bad, mx);
                }
            }
        }
    } else {
        for (int base = 0; base < n4; base += 4 * SGD_THREADS) {
            float v[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * SGD_THREADS + tid;
                if (i < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[k][e] = x[4 * i + e];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = base + k * SGD_THREADS + tid;
                if (i < n4) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) sumsq_take<MAX>(v[k][e], a[e], bad, mx);
                }
            }
        }
    }
    if (tid == (n4 & (SGD_THREADS - 1)))                                    // the n % 4 elements of the last, partial group of four: its owner's last
        for (int e = 0; e < (n & 3); ++e) sumsq_take<MAX>(x[4 * n4 + e], a[e], bad, mx);
    const double s = wave_sum_xor(__dadd_rn(__dadd_rn(a[0], a[1]), __dadd_rn(a[2], a[3])));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d, WAVE);
    if (MAX) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float o = __shfl_xor(mx, d, WAVE);
            if (o > mx) mx = o;
        }
    }
    bad_out = bad;
    max_out = mx;
    return s;
}

__device__ __forceinline__ double sumsq_block4(const double *ws) { return __dadd_rn(__dadd_rn(__dadd_rn(ws[0], ws[1]), ws[2]), ws[3]); }
