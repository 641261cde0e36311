// resample_dev.h -- the arithmetic of Pillow's 8-bit separable bilinear resampler: the window size, one output index's coefficient
// window in fp64 (IEEE +,-,*,/ only -> the same integers as the CPU), one 3-channel window sum, the clip.  Everything past the
// coefficients is 32-bit integer arithmetic, so every user of these functions produces Pillow's bytes.  The transforms reach them
// through input_dev.h (the window table of an axis, one output pixel of a pass).
#pragma once
#include "frcnn_common.h"
#include <cmath>

#define RS_BITS 22

// taps per output index: (int)ceil(max(in / out, 1)) * 2 + 1
static inline int rs_ksize_host(int in_size, int out_size)
{
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(fs) * 2 + 1;
}

#ifdef __HIPCC__

// Output index i of an in_size -> out_size resize: bounds[2i] = first source index, bounds[2i + 1] = number of taps (<= the window size of
// this shape), kk[i * ks .. i * ks + ks) = the 22-bit fixed-point weights, zero past the taps.  ks is the row stride of the table: at
// least the window size of the shape (a table sized for a larger shape may hold a smaller one).
// rs_coeffs_at writes the window of output index i to a row of the caller's choice (bounds2[0..2), kk_row[0..ks)).
__device__ __forceinline__ void rs_coeffs_at(int i, int in_size, int out_size, int ks, int32_t *__restrict__ bounds2, int32_t *__restrict__ kk_row)
{
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double center = 0.0 + ((double)i + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double a = ((double)(x + xmin) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < ks; ++x) {
        double v = 0.0;
        if (x < xmax) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            v = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) v = v / ww;
        }
        kk_row[x] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << RS_BITS)) : (int32_t)(0.5 + v * (double)(1 << RS_BITS));
    }
    bounds2[0] = xmin;
    bounds2[1] = xmax;
}

__device__ __forceinline__ uint8_t rs_clip8(int32_t v)
{
    v >>= RS_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One output pixel: n taps over RGB pixels that lie `step` bytes apart (3 along a row, -3 along a mirrored row, 3 * width down a column),
// the first at p; rounded and clipped to uint8 like Pillow.
__device__ __forceinline__ void rs_window_rgb(const uint8_t *__restrict__ p, ptrdiff_t step, int n, const int32_t *__restrict__ k, uint8_t out[3])
{
    int32_t s0 = 1 << (RS_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < n; ++x, p += step) {
        const int32_t c = k[x];
        s0 += (int32_t)p[0] * c; s1 += (int32_t)p[1] * c; s2 += (int32_t)p[2] * c;
    }
    out[0] = rs_clip8(s0); out[1] = rs_clip8(s1); out[2] = rs_clip8(s2);
}

#endif  // __HIPCC__
