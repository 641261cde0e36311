// input_dev.h -- what the transforms of the device input stage (preprocess.hip, mosaic.hip, photometric.hip, crop.hip) share, one copy each:
// the host checks of a frame's sides and of two buffers' overlap, the window table of one axis of one resize with
// its two device users (fill a row, produce one output pixel of a pass), the clip of a box to a region, and one step of the ordered
// compaction of box rows.  The resampler's arithmetic itself stays in resample_dev.h.
#pragma once
#include "frcnn_host.h"
#include "resample_dev.h"

#define IN_SIDE_MAX 32767                 // a frame side: 32767^2 pixels < 2^30, and 3 * 32767^2 bytes index in 32 bits

static inline bool in_side_ok(int v) { return v >= 1 && v <= IN_SIDE_MAX; }

// do [a, a + na) and [b, b + nb) share a byte?  A NULL buffer overlaps nothing.
static inline bool in_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// The window table of one axis of one resize: row r holds one output index's window, b[2r] = its first source index, b[2r + 1] = its
// number of taps (<= ks), k[r * ks .. r * ks + ks) = the weights (resample_dev.h).  Which output index a row belongs to is the owner's
// business: preprocess.hip and mosaic.hip keep row i for index i, crop.hip keeps the region's indices only.
struct RsAxis { int32_t *b, *k; int ks; };

static inline RsAxis rs_axis_take(WsCarver &c, int in_size, int out_size, int n_rows)
{
    RsAxis a;
    a.ks = rs_ksize_host(in_size, out_size);
    a.b = c.get<int32_t>((size_t)n_rows * 2);
    a.k = c.get<int32_t>((size_t)n_rows * a.ks);
    return a;
}

#ifdef __HIPCC__

// row `row` of the table := the window of output index i of an in_size -> out_size resize (in_size / out_size no larger than the
// shape the table's ks was taken for)
__device__ __forceinline__ void rs_axis_coeffs(const RsAxis &a, int row, int i, int in_size, int out_size)
{
    rs_coeffs_at(i, in_size, out_size, a.ks, a.b + 2 * row, a.k + (size_t)row * a.ks);
}

// One output pixel of a horizontal or vertical pass through window `row`: source index s of that axis lies at base + (s - shift) * step
// bytes (step: 3 along a row, -3 along a mirrored row, 3 * width down a column; shift: the source index base stands for, 0 for a whole
// frame).  The caller answers for the window lying inside what base addresses.
__device__ __forceinline__ void rs_pass_rgb(const RsAxis &a, int row, const uint8_t *base, ptrdiff_t step, int shift, uint8_t px[3])
{
    rs_window_rgb(base + (ptrdiff_t)(a.b[2 * row] - shift) * step, step, a.b[2 * row + 1], a.k + (size_t)row * a.ks, px);
}

__device__ __forceinline__ void rs_pass_px(const RsAxis &a, int row, const uint8_t *base, ptrdiff_t step, int shift, uint8_t *dst)
{
    uint8_t px[3];
    rs_pass_rgb(a, row, base, step, shift, px);
    dst[0] = px[0]; dst[1] = px[1]; dst[2] = px[2];
}

// The reference's crop of one box to the region (i, j, h, w), operation for operation in binary32 (datasets/transforms_.py:156-161,
// new_datasets/transforms.py:30-32,48-49): shift, min with the region's size, clamp at 0 -> *c; kept when it still has an area.
// NaN coordinates stay NaN and compare false.
__device__ __forceinline__ bool in_clip_box(float4 b, float fi, float fj, float fh, float fw, float4 *c)
{
    float x1 = tmin(b.x - fj, fw), y1 = tmin(b.y - fi, fh), x2 = tmin(b.z - fj, fw), y2 = tmin(b.w - fi, fh);
    x1 = x1 < 0.0f ? 0.0f : x1; y1 = y1 < 0.0f ? 0.0f : y1; x2 = x2 < 0.0f ? 0.0f : x2; y2 = y2 < 0.0f ? 0.0f : y2;
    *c = make_float4(x1, y1, x2, y2);
    return x2 > x1 && y2 > y1;
}

// One step of the ordered compaction of rows by ONE workgroup of 256, one row per thread: ballot + popcount inside a wave, the four
// wave totals through s_wave[4] (LDS), `base` = the rows kept so far, the same in every thread.  Returns the output slot of this
// thread's row (meaningful where keep) and advances base by the step's kept rows.  Both barriers are in here, so EVERY thread of the
// 256 must make the call, in a loop whose trip count is uniform across the workgroup; threads without a row pass keep = false.
__device__ __forceinline__ int in_compact_slot(bool keep, int &base, int *s_wave)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int slot = base + __popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < wave; ++q) slot += s_wave[q];
    base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();                                                  // s_wave is rewritten by the next step only after every thread has read it
    return slot;
}

#endif  // __HIPCC__
