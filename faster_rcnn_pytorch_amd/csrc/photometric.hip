// photometric.hip -- the two functions of the reference's richer training recipe (datasets/build.py:28-42) that change pixels without
// changing what the host knows about shapes, for one uint8 HWC frame already in HBM:
//   photometric_distort_  (datasets/transforms_.py:38-58; RandomPhotoDistortion :240-247): brightness, contrast, saturation and hue, each
//                         once, in a shuffled order; every op ends in a real uint8 image (photometric_dev.h: Pillow's arithmetic)
//   zoom_out_             (transforms_.py:130-147; RandomZoomOut :291-299): the frame pasted into a larger canvas filled with its
//                         per-channel MEDIAN, boxes shifted
// frcnn_photometric: two launches, whatever the plan in device memory says.  Contrast blends towards the mean luma of the image AS IT
// STANDS when contrast is applied, a global reduction in the middle of a per-pixel chain:
//   pm_sum_kernel    runs the ops in front of contrast in registers and sums L exactly (uint64: 32767^2 * 255 needs 36 bits); one
//                    partial sum per workgroup, every one of them written in every call that reads them -- no atomics, no counter to zero
//   pm_apply_kernel  adds the partials up (integers: any order gives the same sum), forms the mean, recomputes the ops in front of
//                    contrast from the source and applies contrast and what follows.  No intermediate image is written.
// frcnn_zoom_out: three launches, kernels only:
//   zo_hist_kernel   3 x 256 bins, one LDS copy per wave (integer adds); every workgroup stores its own 768 counts to HBM -- like the
//                    luma partials: all of them written in every call, nothing to zero, no atomics outside LDS
//   zo_median_kernel one workgroup merges the workgroups' counts, then the first level whose cumulative count exceeds count / 2
//                    (Pillow's rule), per channel; the shifted boxes
//   zo_fill_kernel   every canvas pixel written once: the source pixel inside the paste, the median outside
// Pixels are 3 bytes: every lane handles 4 pixels = 3 whole dwords (both frames start 4-byte aligned and are dense, so group g of the
// flat pixel list is dwords 3g .. 3g+2 whatever the width), a wave 768 contiguous bytes; the up to 3 pixels left over go byte by byte.
// Grid-stride loops over a grid sized from the CU count.
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
FRCNN_LAYOUT_STAMP(photometric);
#include "photometric_dev.h"
#include "input_dev.h"

#define PM_MAX_BLOCKS 4096                // partial sums the workspace holds; the grid is min(work, 8 per CU, this)
#define ZO_HIST_BLOCKS 128                // workgroups of the histogram pass = rows of counts the workspace holds
#define ZO_WS_PART 16                     // the workspace in dwords: [0, 3) the medians, from here [ZO_HIST_BLOCKS][768] counts

__device__ __forceinline__ PmPixel pm_load_px(const uint8_t *p) { PmPixel x; x.r = p[0]; x.g = p[1]; x.b = p[2]; return x; }
__device__ __forceinline__ void pm_store_px(uint8_t *p, PmPixel x) { p[0] = (uint8_t)x.r; p[1] = (uint8_t)x.g; p[2] = (uint8_t)x.b; }

// the sum of one value per thread over a workgroup of 256, valid in thread 0
__device__ __forceinline__ uint64_t pm_block_sum(uint64_t v, uint64_t *s_wave)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = v;
    __syncthreads();
    return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ __launch_bounds__(256) void pm_sum_kernel(const uint32_t *__restrict__ src, uint32_t npix, const int32_t *__restrict__ plan,
                                                     uint64_t *__restrict__ partial)
{
    __shared__ uint64_t s_wave[4];
    const PmPlan P = pm_decode(plan);
    if (P.contrast_at < 0) return;                                    // nothing reads the partials then
    const uint32_t ngroups = npix >> 2;
    uint64_t acc = 0;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < ngroups; g += gridDim.x * 256u) {
        const uint32_t *q = src + 3 * (size_t)g;
        PmPixel px[4];
        pm_unpack4(q[0], q[1], q[2], px);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += pm_luma(pm_apply(P, 0, P.contrast_at, 0, px[k]));
    }
    if (blockIdx.x == 0 && threadIdx.x < (npix & 3u)) {
        const uint32_t i = (ngroups << 2) + threadIdx.x;
        acc += pm_luma(pm_apply(P, 0, P.contrast_at, 0, pm_load_px((const uint8_t *)src + 3 * (size_t)i)));
    }
    const uint64_t total = pm_block_sum(acc, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void pm_apply_kernel(const uint32_t *__restrict__ src, uint32_t npix, const int32_t *__restrict__ plan,
                                                       const uint64_t *__restrict__ partial, int n_partial, uint32_t *__restrict__ out)
{
    __shared__ uint64_t s_wave[4];
    const PmPlan P = pm_decode(plan);
    uint32_t mean = 0;
    if (P.contrast_at >= 0) {                                         // uniform: the plan is one for the whole grid
        uint64_t acc = 0;
        for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
        mean = pm_mean_level(pm_block_sum(acc, s_wave), (uint64_t)npix);
    }
    const uint32_t ngroups = npix >> 2;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < ngroups; g += gridDim.x * 256u) {
        const uint32_t *q = src + 3 * (size_t)g;
        PmPixel px[4];
        pm_unpack4(q[0], q[1], q[2], px);
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = pm_apply(P, 0, P.n, mean, px[k]);
        uint32_t w0, w1, w2;
        pm_pack4(px, &w0, &w1, &w2);
        uint32_t *o = out + 3 * (size_t)g;
        o[0] = w0; o[1] = w1; o[2] = w2;
    }
    if (blockIdx.x == 0 && threadIdx.x < (npix & 3u)) {
        const size_t i = ((size_t)ngroups << 2) + threadIdx.x;
        pm_store_px((uint8_t *)out + 3 * i, pm_apply(P, 0, P.n, mean, pm_load_px((const uint8_t *)src + 3 * i)));
    }
}

// ---- zoom-out ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zo_hist_kernel(const uint32_t *__restrict__ src, uint32_t npix, uint32_t *__restrict__ part)
{
    __shared__ uint32_t s_h[4][768];
    for (int i = threadIdx.x; i < 4 * 768; i += 256) (&s_h[0][0])[i] = 0;
    __syncthreads();
    uint32_t *h = s_h[threadIdx.x >> 6];
    const uint32_t ngroups = npix >> 2;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < ngroups; g += gridDim.x * 256u) {
        const uint32_t *q = src + 3 * (size_t)g;
        PmPixel px[4];
        pm_unpack4(q[0], q[1], q[2], px);
#pragma unroll
        for (int k = 0; k < 4; ++k) { atomicAdd(&h[px[k].r], 1u); atomicAdd(&h[256 + px[k].g], 1u); atomicAdd(&h[512 + px[k].b], 1u); }
    }
    if (blockIdx.x == 0 && threadIdx.x < (npix & 3u)) {
        const PmPixel p = pm_load_px((const uint8_t *)src + 3 * (((size_t)ngroups << 2) + threadIdx.x));
        atomicAdd(&h[p.r], 1u); atomicAdd(&h[256 + p.g], 1u); atomicAdd(&h[512 + p.b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 768; i += 256) part[768 * (size_t)blockIdx.x + i] = s_h[0][i] + s_h[1][i] + s_h[2][i] + s_h[3][i];
}

// one workgroup: the workgroups' counts merged (a frame has at most 32767^2 < 2^30 pixels: 32 bits hold every sum), the three medians, then boxes + float32(left, top, left, top) (transforms_.py:145)
__global__ __launch_bounds__(256) void zo_median_kernel(const uint32_t *__restrict__ part, int n_part, uint32_t npix, uint32_t *__restrict__ median,
                                                        const float4 *__restrict__ boxes, int64_t n, float fleft, float ftop,
                                                        float4 *__restrict__ boxes_out)
{
    __shared__ uint32_t s_h[768];
    for (int i = threadIdx.x; i < 768; i += 256) {
        uint32_t v = 0;
        for (int b = 0; b < n_part; ++b) v += part[768 * (size_t)b + i];
        s_h[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t half = npix >> 1;
        uint32_t cum = 0, level = 255;
        for (int j = 0; j < 256; ++j) {
            cum += s_h[256 * threadIdx.x + j];
            if (cum > half) { level = (uint32_t)j; break; }
        }
        median[threadIdx.x] = level;
    }
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float4 b = boxes[i];
        boxes_out[i] = make_float4(b.x + fleft, b.y + ftop, b.z + fleft, b.w + ftop);
    }
}

// 12 bytes from any byte address: the aligned dwords that hold them, shifted into place.  Every dword read holds at least one of the
// 12 bytes, so nothing outside the words the frame itself occupies is touched.
__device__ __forceinline__ void zo_load12(const uint8_t *p, uint32_t *w0, uint32_t *w1, uint32_t *w2)
{
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3u) * 8u;
    const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
    if (sh == 0) { *w0 = d0; *w1 = d1; *w2 = d2; return; }
    const uint32_t d3 = q[3];
    *w0 = (d0 >> sh) | (d1 << (32u - sh)); *w1 = (d1 >> sh) | (d2 << (32u - sh)); *w2 = (d2 >> sh) | (d3 << (32u - sh));
}

__global__ __launch_bounds__(256) void zo_fill_kernel(const uint8_t *__restrict__ src, int h, int w, int new_w, uint32_t ncanvas, int top, int left,
                                                      const uint32_t *__restrict__ median, uint32_t *__restrict__ canvas)
{
    PmPixel m;
    m.r = median[0] & 255u; m.g = median[1] & 255u; m.b = median[2] & 255u;
    const uint32_t ngroups = ncanvas >> 2;
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < ngroups; g += gridDim.x * 256u) {
        const uint32_t p0 = g << 2;
        int y = (int)(p0 / (uint32_t)new_w), x = (int)(p0 - (uint32_t)y * (uint32_t)new_w);
        uint32_t w0, w1, w2;
        if (x + 3 < new_w && y >= top && y < top + h && x >= left && x + 3 < left + w) {              // four pixels of one source row
            zo_load12(src + ((size_t)(y - top) * (size_t)w + (size_t)(x - left)) * 3, &w0, &w1, &w2);
        } else {
            PmPixel px[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = y >= top && y < top + h && x >= left && x < left + w;
                px[k] = in ? pm_load_px(src + ((size_t)(y - top) * (size_t)w + (size_t)(x - left)) * 3) : m;
                if (++x == new_w) { x = 0; ++y; }
            }
            pm_pack4(px, &w0, &w1, &w2);
        }
        uint32_t *o = canvas + 3 * (size_t)g;
        o[0] = w0; o[1] = w1; o[2] = w2;
    }
    if (blockIdx.x == 0 && threadIdx.x < (ncanvas & 3u)) {
        const uint32_t i = (ngroups << 2) + threadIdx.x;
        const int y = (int)(i / (uint32_t)new_w), x = (int)(i - (uint32_t)y * (uint32_t)new_w);
        const bool in = y >= top && y < top + h && x >= left && x < left + w;
        pm_store_px((uint8_t *)canvas + 3 * (size_t)i, in ? pm_load_px(src + ((size_t)(y - top) * (size_t)w + (size_t)(x - left)) * 3) : m);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// workgroups of 256 for `groups` four-pixel groups: at most 8 per CU of the current device, at most PM_MAX_BLOCKS, at least 1
static int pm_grid(uint32_t groups, unsigned *grid)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return frcnn_set_error(FRCNN_ERR_LAUNCH, "photometric: no current HIP device");
    const int cus = frcnn_cu_count();
    if (cus < 1) return frcnn_set_error(FRCNN_ERR_LAUNCH, "photometric: cannot read the CU count of device %d", dev);
    uint32_t need = (groups + 255u) / 256u, cap = 8u * (uint32_t)cus;
    if (cap > PM_MAX_BLOCKS) cap = PM_MAX_BLOCKS;
    if (need > cap) need = cap;
    *grid = need < 1u ? 1u : need;
    return FRCNN_OK;
}

FRCNN_EXPORT size_t frcnn_photometric_workspace(int h, int w)
{
    if (!in_side_ok(h) || !in_side_ok(w)) return 0;
    return PM_MAX_BLOCKS * sizeof(uint64_t);
}

FRCNN_EXPORT int frcnn_photometric(const uint8_t *src_hwc, int h, int w, const int32_t *plan_dev, uint8_t *out_hwc, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(src_hwc && plan_dev && out_hwc && workspace, "photometric: NULL pointer");
    FRCNN_REQUIRE(in_side_ok(h) && in_side_ok(w), "photometric: bad shape %d x %d (sides of 1 .. 32767)", h, w);
    const size_t bytes = (size_t)h * (size_t)w * 3;
    FRCNN_REQUIRE(((uintptr_t)src_hwc & 3) == 0 && ((uintptr_t)out_hwc & 3) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)plan_dev & 3) == 0,
                  "photometric: src and out must be 4-byte aligned, the workspace 8-byte aligned");
    FRCNN_REQUIRE(!in_overlap(src_hwc, bytes, out_hwc, bytes), "photometric: out overlaps src (pass 2 reads the source again)");
    const size_t need = frcnn_photometric_workspace(h, w);
    if (workspace_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "photometric: workspace %zu < %zu", workspace_bytes, need);
    const uint32_t npix = (uint32_t)h * (uint32_t)w;
    unsigned grid = 1;
    const int rc = pm_grid(npix >> 2, &grid);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(pm_sum_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t *)src_hwc, npix, plan_dev, (uint64_t *)workspace);
    FRCNN_LAUNCH(pm_apply_kernel, dim3(grid), dim3(256), 0, s, (const uint32_t *)src_hwc, npix, plan_dev, (const uint64_t *)workspace, (int)grid,
                 (uint32_t *)out_hwc);
    FRCNN_CHECK_LAUNCH("photometric kernels");
    return FRCNN_OK;
}

FRCNN_EXPORT size_t frcnn_zoom_out_workspace(int h, int w, int new_h, int new_w)
{
    if (!in_side_ok(h) || !in_side_ok(w) || !in_side_ok(new_h) || !in_side_ok(new_w) || new_h < h || new_w < w) return 0;
    return (ZO_WS_PART + (size_t)ZO_HIST_BLOCKS * 768) * sizeof(uint32_t);
}

FRCNN_EXPORT int frcnn_zoom_out(const uint8_t *src_hwc, int h, int w, int new_h, int new_w, int top, int left, const float *boxes, int64_t n,
                                uint8_t *canvas, float *boxes_out, void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(src_hwc && canvas && workspace, "zoom_out: NULL pointer");
    FRCNN_REQUIRE(n >= 0 && (n == 0 || (boxes && boxes_out)), "zoom_out: NULL box pointer with %lld boxes (or a negative count)", (long long)n);
    FRCNN_REQUIRE(in_side_ok(h) && in_side_ok(w) && in_side_ok(new_h) && in_side_ok(new_w),
                  "zoom_out: bad shape %d x %d -> %d x %d (sides of 1 .. 32767, the canvas included)", h, w, new_h, new_w);
    FRCNN_REQUIRE(new_h >= h && new_w >= w, "zoom_out: the canvas %d x %d is smaller than the frame %d x %d", new_h, new_w, h, w);
    FRCNN_REQUIRE(top >= 0 && left >= 0 && top <= new_h - h && left <= new_w - w,
                  "zoom_out: the paste at (top %d, left %d) leaves the canvas (top <= %d, left <= %d)", top, left, new_h - h, new_w - w);
    FRCNN_REQUIRE(((uintptr_t)src_hwc & 3) == 0 && ((uintptr_t)canvas & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                  "zoom_out: src, canvas and workspace must be 4-byte aligned");
    FRCNN_REQUIRE(n == 0 || (((uintptr_t)boxes & 15) == 0 && ((uintptr_t)boxes_out & 15) == 0), "zoom_out: boxes and boxes_out must be 16-byte aligned");
    const size_t sbytes = (size_t)h * (size_t)w * 3, cbytes = (size_t)new_h * (size_t)new_w * 3;
    FRCNN_REQUIRE(!in_overlap(src_hwc, sbytes, canvas, cbytes), "zoom_out: the canvas overlaps src");
    const size_t need = frcnn_zoom_out_workspace(h, w, new_h, new_w);
    if (workspace_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "zoom_out: workspace %zu < %zu", workspace_bytes, need);
    const uint32_t npix = (uint32_t)h * (uint32_t)w, ncanvas = (uint32_t)new_h * (uint32_t)new_w;
    unsigned gh = 1, gf = 1;
    int rc = pm_grid(npix >> 2, &gh);
    if (!rc) rc = pm_grid(ncanvas >> 2, &gf);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *median = (uint32_t *)workspace, *part = median + ZO_WS_PART;
    if (gh > ZO_HIST_BLOCKS) gh = ZO_HIST_BLOCKS;
    FRCNN_LAUNCH(zo_hist_kernel, dim3(gh), dim3(256), 0, s, (const uint32_t *)src_hwc, npix, part);
    FRCNN_LAUNCH(zo_median_kernel, dim3(1), dim3(256), 0, s, (const uint32_t *)part, (int)gh, npix, median, (const float4 *)boxes, n, (float)left, (float)top,
                 (float4 *)boxes_out);
    FRCNN_LAUNCH(zo_fill_kernel, dim3(gf), dim3(256), 0, s, src_hwc, h, w, new_w, ncanvas, top, left, (const uint32_t *)median, (uint32_t *)canvas);
    FRCNN_CHECK_LAUNCH("zoom_out kernels");
    return FRCNN_OK;
}
