// mosaic.hip -- the reference's --mosaic_transform (config.py:16; datasets/voc_dataset.py:145-156, datasets/coco_dataset.py:154-157;
// datasets/mosaic_transform.py:7-26,70-95 on datasets/transforms_.py:61-127,150-178,278-288) for four uint8 HWC frames already in HBM:
//   per tile  Resize(size, max_size) -> crop_(region, min_overlap_ratio 0.3) -> Resize((size, size)) -> shift -> paste into a quadrant
// of a 2*size x 2*size canvas, the four box lists compacted into one.  crop_ hands back the UNCROPPED frame and ALL its boxes when no
// box survives the crop (transforms_.py:174-176), so which pixels a tile is made of depends on its boxes: that decision is taken by
// the box kernel and stays in device memory, where the image kernels read it.  Six launches, whatever the boxes say:
//   mosaic_boxes_kernel   : ONE workgroup walks the four tiles in order: pass 1 asks whether any box survives, pass 2 compacts the
//                           survivors (or all boxes) in order, 256 at a time (in_compact_slot, one running base across chunks and
//                           tiles); writes the region used, the flag, the count, zeros past it
//   mosaic_coeffs_kernel  : Pillow's windows of both resizes of every tile; the second resize's come from the region in device memory
//   mosaic_h1/v1_kernel   : first resize, only the columns / rows the region needs (outputs are independent per pixel) -> a real
//                           uint8 image, as the reference has between its two resizes
//   mosaic_h2/v2_kernel   : second resize of the region as an image of its own, the vertical pass storing into the canvas quadrant
// The tile is a grid axis; grids are sized for the whole resized frame (the worst of the two possible regions) and workgroups past the
// region leave at once.  Byte gathers through short windows: latency and launch bound at these sizes, not bandwidth.
// Box arithmetic is the reference's, operation for operation, in binary32 (-ffp-contract=off).
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
FRCNN_LAYOUT_STAMP(mosaic);
#include "input_dev.h"

struct MosaicTile {
    const uint8_t *src;
    int h, w, H1, W1;                     // the source frame and its first resize
    int reg[4];                           // the caller's crop (i, j, h, w) in the resized frame
    float r1w, r1h;                       // transforms_.py:118-125: new / old, formed in double
    float r2w[2], r2h[2];                 // the second resize's ratios: [0] the crop was taken, [1] it was not
    int box_lo, box_hi;                   // this tile's rows of the tile-major box list
    RsAxis x1, y1, x2, y2;                // both resizes' window tables, row = output index (second resize: strides for the worst case, the whole frame)
    uint8_t *tmp1, *img1, *tmp2;          // [h, W1, 3], [H1, W1, 3] (both in frame coordinates), [H1, size, 3] (region rows)
};
struct MosaicDesc { MosaicTile t[4]; int size; int32_t *regions; /* [4][4] device: the region each tile used */ };
static_assert(sizeof(MosaicDesc) <= 4096, "MosaicDesc must fit the kernarg segment");

// crop_ (transforms_.py:155-168) for one resized box: the clipped box and whether it is kept
__device__ __forceinline__ bool mosaic_crop_keep(float4 b, float fi, float fj, float fh, float fw, float4 *c)
{
    const bool keep = in_clip_box(b, fi, fj, fh, fw, c);                                                         // :156-161
    const float bw = b.z - b.x, bh = b.w - b.y, cw = c->z - c->x, ch = c->w - c->y;                             // :165-166
    return keep && (cw * ch) / (bw * bh) > 0.3f;                                                                 // :167 (NaN compares false)
}

__global__ __launch_bounds__(256) void mosaic_boxes_kernel(MosaicDesc d, const float4 *__restrict__ boxes, const int64_t *__restrict__ labels, int n_total,
                                                          float4 *__restrict__ boxes_out, int64_t *__restrict__ labels_out,
                                                          int32_t *__restrict__ count_dev, uint8_t *__restrict__ fallback_dev)
{
    __shared__ int s_any, s_wave[4];
    const int tid = threadIdx.x;
    const float fsize = (float)d.size;
    int base = 0;                                                     // live rows so far: the same in every thread
    for (int t = 0; t < 4; ++t) {
        const MosaicTile &T = d.t[t];
        const float fi = (float)T.reg[0], fj = (float)T.reg[1], fh = (float)T.reg[2], fw = (float)T.reg[3];
        if (tid == 0) s_any = 0;
        __syncthreads();
        bool any = false;
        for (int i = T.box_lo + tid; i < T.box_hi; i += 256) {
            const float4 b = boxes[i];
            float4 c;
            any |= mosaic_crop_keep(make_float4(b.x * T.r1w, b.y * T.r1h, b.z * T.r1w, b.w * T.r1h), fi, fj, fh, fw, &c);
        }
        if (any) s_any = 1;
        __syncthreads();
        const int fb = s_any ? 0 : 1;                                 // transforms_.py:174-176: nothing kept -> the uncropped frame, all boxes
        __syncthreads();                                              // s_any is reset for the next tile only after every thread has read it
        if (tid == 0) {
            int32_t *r = d.regions + 4 * t;
            r[0] = fb ? 0 : T.reg[0]; r[1] = fb ? 0 : T.reg[1]; r[2] = fb ? T.H1 : T.reg[2]; r[3] = fb ? T.W1 : T.reg[3];
            fallback_dev[t] = (uint8_t)fb;
        }
        const float r2w = T.r2w[fb], r2h = T.r2h[fb];
        const float sx = (t & 1) ? fsize : 0.0f, sy = (t >> 1) ? fsize : 0.0f;       // mosaic_transform.py:82-85
        for (int c0 = T.box_lo; c0 < T.box_hi; c0 += 256) {            // uniform trip count: every thread makes every in_compact_slot call
            const int i = c0 + tid;
            bool keep = false;
            float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < T.box_hi) {
                const float4 b = boxes[i];
                const float4 b1 = make_float4(b.x * T.r1w, b.y * T.r1h, b.z * T.r1w, b.w * T.r1h);
                float4 c;
                keep = mosaic_crop_keep(b1, fi, fj, fh, fw, &c) || fb;
                o = fb ? b1 : c;
            }
            const int off = in_compact_slot(keep, base, s_wave);
            if (keep) {
                boxes_out[off] = make_float4(o.x * r2w + sx, o.y * r2h + sy, o.z * r2w + sx, o.w * r2h + sy);
                labels_out[off] = labels[i];
            }
        }
    }
    for (int i = base + tid; i < n_total; i += 256) { boxes_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); labels_out[i] = 0; }
    if (tid == 0) *count_dev = base;
}

// the region a tile uses, as the box kernel left it; false when it is not a region of the tile's resized frame (then nothing is addressed by it)
__device__ __forceinline__ bool mosaic_region(const MosaicDesc &d, int t, int *ri, int *rj, int *rh, int *rw)
{
    const int32_t *r = d.regions + 4 * t;
    *ri = r[0]; *rj = r[1]; *rh = r[2]; *rw = r[3];
    return *ri >= 0 && *rj >= 0 && *rh >= 1 && *rw >= 1 && *rh <= d.t[t].H1 - *ri && *rw <= d.t[t].W1 - *rj;
}

__global__ __launch_bounds__(256) void mosaic_coeffs_kernel(MosaicDesc d)
{
    const int t = blockIdx.y;
    const MosaicTile &T = d.t[t];
    int ri, rj, rh, rw;
    if (!mosaic_region(d, t, &ri, &rj, &rh, &rw)) return;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < T.W1) { rs_axis_coeffs(T.x1, i, i, T.w, T.W1); return; }
    i -= T.W1;
    if (i < T.H1) { rs_axis_coeffs(T.y1, i, i, T.h, T.H1); return; }
    i -= T.H1;
    if (i < d.size) { rs_axis_coeffs(T.x2, i, i, rw, d.size); return; }      // rw <= W1: the window fits the stride
    i -= d.size;
    if (i < d.size) rs_axis_coeffs(T.y2, i, i, rh, d.size);
}

// first resize, horizontal: the region's columns, on the source rows its rows' windows reach
__global__ __launch_bounds__(256) void mosaic_h1_kernel(MosaicDesc d)
{
    const int t = blockIdx.z;
    const MosaicTile &T = d.t[t];
    int ri, rj, rh, rw;
    if (!mosaic_region(d, t, &ri, &rj, &rh, &rw)) return;
    const int x0 = blockIdx.x * 256 + threadIdx.x;
    const int ylo = T.y1.b[2 * ri], yhi = T.y1.b[2 * (ri + rh - 1)] + T.y1.b[2 * (ri + rh - 1) + 1];
    if (x0 >= rw || (int)blockIdx.y >= yhi - ylo) return;
    const int xx = rj + x0, y = ylo + blockIdx.y;
    if (y < 0 || y >= T.h) return;
    rs_pass_px(T.x1, xx, T.src + (size_t)y * T.w * 3, 3, 0, T.tmp1 + ((size_t)y * T.W1 + xx) * 3);
}

// first resize, vertical: the region's pixels of the resized uint8 frame
__global__ __launch_bounds__(256) void mosaic_v1_kernel(MosaicDesc d)
{
    const int t = blockIdx.z;
    const MosaicTile &T = d.t[t];
    int ri, rj, rh, rw;
    if (!mosaic_region(d, t, &ri, &rj, &rh, &rw)) return;
    const int x0 = blockIdx.x * 256 + threadIdx.x;
    if (x0 >= rw || (int)blockIdx.y >= rh) return;
    const int xx = rj + x0, yy = ri + blockIdx.y;
    rs_pass_px(T.y1, yy, T.tmp1 + (size_t)xx * 3, (ptrdiff_t)T.W1 * 3, 0, T.img1 + ((size_t)yy * T.W1 + xx) * 3);
}

// second resize, horizontal: the region as an image of its own, [rh, rw] -> [rh, size]
__global__ __launch_bounds__(256) void mosaic_h2_kernel(MosaicDesc d)
{
    const int t = blockIdx.z;
    const MosaicTile &T = d.t[t];
    int ri, rj, rh, rw;
    if (!mosaic_region(d, t, &ri, &rj, &rh, &rw)) return;
    const int xx = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (xx >= d.size || r >= rh) return;
    rs_pass_px(T.x2, xx, T.img1 + ((size_t)(ri + r) * T.W1 + rj) * 3, 3, 0, T.tmp2 + ((size_t)r * d.size + xx) * 3);      // the region is img1's sub-image at (ri, rj)
}

// second resize, vertical, stored into the tile's quadrant (mosaic_transform.py:15-26,88-91: equal tiles, so the centre offsets are 0)
__global__ __launch_bounds__(256) void mosaic_v2_kernel(MosaicDesc d, uint8_t *__restrict__ canvas)
{
    const int t = blockIdx.z;
    const MosaicTile &T = d.t[t];
    int ri, rj, rh, rw;
    if (!mosaic_region(d, t, &ri, &rj, &rh, &rw)) return;
    const int xx = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
    if (xx >= d.size) return;
    const size_t cy = (size_t)(t >> 1) * d.size + yy, cx = (size_t)(t & 1) * d.size + xx;
    rs_pass_px(T.y2, yy, T.tmp2 + (size_t)xx * 3, (ptrdiff_t)d.size * 3, 0, canvas + (cy * (2 * (size_t)d.size) + cx) * 3);
}

// resize_'s size logic (transforms_.py:93-114), in its own order of double operations; max_size <= 0: no cap
static void mosaic_first_size(int h, int w, int size, int max_size, int *H1, int *W1)
{
    if (max_size > 0) {
        const double lo = (double)(h < w ? h : w), hi = (double)(h < w ? w : h);
        if ((double)size / lo * hi > (double)max_size) size = (int)std::nearbyint((double)max_size / hi * lo);      // round(): half to even
    }
    if ((w <= h && w == size) || (h <= w && h == size)) { *H1 = h; *W1 = w; }
    else if (w < h) { *W1 = size; *H1 = (int)((double)((int64_t)size * h) / (double)w); }
    else { *H1 = size; *W1 = (int)((double)((int64_t)size * w) / (double)h); }
}

static bool mosaic_shapes_ok(const int32_t *src_hw, int size, int max_size, int H1[4], int W1[4])
{
    if (!src_hw || !in_side_ok(size) || !in_side_ok(2 * size)) return false;
    for (int t = 0; t < 4; ++t) {
        const int h = src_hw[2 * t], w = src_hw[2 * t + 1];
        if (!in_side_ok(h) || !in_side_ok(w)) return false;
        mosaic_first_size(h, w, size, max_size, &H1[t], &W1[t]);
        if (!in_side_ok(H1[t]) || !in_side_ok(W1[t])) return false;
    }
    return true;
}

static size_t mosaic_ws_layout(void *base, const int32_t *src_hw, const int H1[4], const int W1[4], int size, MosaicDesc *d)
{
    WsCarver c(base);
    d->size = size;
    d->regions = c.get<int32_t>(16);
    for (int t = 0; t < 4; ++t) {
        MosaicTile &T = d->t[t];
        T.h = src_hw[2 * t]; T.w = src_hw[2 * t + 1]; T.H1 = H1[t]; T.W1 = W1[t];
        T.x1 = rs_axis_take(c, T.w, T.W1, T.W1); T.y1 = rs_axis_take(c, T.h, T.H1, T.H1);
        T.x2 = rs_axis_take(c, T.W1, size, size); T.y2 = rs_axis_take(c, T.H1, size, size);
        T.tmp1 = c.get<uint8_t>((size_t)T.h * T.W1 * 3); T.img1 = c.get<uint8_t>((size_t)T.H1 * T.W1 * 3);
        T.tmp2 = c.get<uint8_t>((size_t)T.H1 * size * 3);
    }
    return c.bytes();
}

FRCNN_EXPORT size_t frcnn_mosaic_workspace(const int32_t *src_hw, int size, int max_size)
{
    int H1[4], W1[4];
    if (!mosaic_shapes_ok(src_hw, size, max_size, H1, W1)) return 0;
    MosaicDesc d;
    return mosaic_ws_layout(nullptr, src_hw, H1, W1, size, &d);
}

FRCNN_EXPORT int frcnn_mosaic(const uint8_t *const src_hwc[4], const int32_t *src_hw, int size, int max_size, const int32_t *regions,
                              const float *boxes, const int64_t *labels, const int32_t *tile_offsets, uint8_t *canvas, float *boxes_out,
                              int64_t *labels_out, int32_t *count_dev, uint8_t *fallback_dev, void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(src_hwc && src_hw && regions && tile_offsets && canvas && count_dev && fallback_dev && workspace, "mosaic: NULL pointer");
    for (int t = 0; t < 4; ++t) FRCNN_REQUIRE(src_hwc[t], "mosaic: NULL source frame %d", t);
    // only the upper limit here, not in_side_ok(): a side < 1 keeps falling through to the 'bad shape' message below
    for (int t = 0; t < 4; ++t)
        FRCNN_REQUIRE(src_hw[2 * t] <= IN_SIDE_MAX && src_hw[2 * t + 1] <= IN_SIDE_MAX, "mosaic: frame %d too large (%d x %d, sides must be < 32768)", t,
                      src_hw[2 * t], src_hw[2 * t + 1]);
    int H1[4], W1[4];
    FRCNN_REQUIRE(mosaic_shapes_ok(src_hw, size, max_size, H1, W1), "mosaic: bad shape (sides >= 1, size >= 1, 2 * size and every resized side < 32768)");
    for (int t = 0; t < 4; ++t) {
        const int32_t *r = regions + 4 * t;
        FRCNN_REQUIRE(r[2] >= 1 && r[3] >= 1, "mosaic: region %d has h = %d, w = %d (both must be >= 1)", t, r[2], r[3]);
        FRCNN_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[2] <= H1[t] - r[0] && r[3] <= W1[t] - r[1],
                      "mosaic: region %d (i %d, j %d, h %d, w %d) is outside its resized frame %d x %d", t, r[0], r[1], r[2], r[3], H1[t], W1[t]);
    }
    FRCNN_REQUIRE(tile_offsets[0] == 0, "mosaic: tile_offsets[0] must be 0");
    for (int t = 0; t < 4; ++t)
        FRCNN_REQUIRE(tile_offsets[t + 1] >= tile_offsets[t], "mosaic: tile_offsets must not decrease (%d after %d)", tile_offsets[t + 1], tile_offsets[t]);
    const int n = tile_offsets[4];
    FRCNN_REQUIRE(n == 0 || (boxes && labels && boxes_out && labels_out), "mosaic: NULL box / label pointer with %d boxes", n);
    MosaicDesc d;
    const size_t need = mosaic_ws_layout(workspace, src_hw, H1, W1, size, &d);
    if (workspace_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "mosaic: workspace %zu < %zu", workspace_bytes, need);
    int hmax = 1, H1max = 1, W1max = 1, rows = 1;
    for (int t = 0; t < 4; ++t) {
        MosaicTile &T = d.t[t];
        const int32_t *r = regions + 4 * t;
        T.src = src_hwc[t];
        for (int q = 0; q < 4; ++q) T.reg[q] = r[q];
        T.r1w = (float)((double)T.W1 / (double)T.w); T.r1h = (float)((double)T.H1 / (double)T.h);
        T.r2w[0] = (float)((double)size / (double)r[3]); T.r2h[0] = (float)((double)size / (double)r[2]);
        T.r2w[1] = (float)((double)size / (double)T.W1); T.r2h[1] = (float)((double)size / (double)T.H1);
        T.box_lo = tile_offsets[t]; T.box_hi = tile_offsets[t + 1];
        hmax = T.h > hmax ? T.h : hmax; H1max = T.H1 > H1max ? T.H1 : H1max; W1max = T.W1 > W1max ? T.W1 : W1max;
        rows = T.W1 + T.H1 + 2 * size > rows ? T.W1 + T.H1 + 2 * size : rows;
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned gw1 = (unsigned)((W1max + 255) / 256), gs = (unsigned)((size + 255) / 256);
    FRCNN_LAUNCH(mosaic_boxes_kernel, dim3(1), dim3(256), 0, s, d, (const float4 *)boxes, labels, n, (float4 *)boxes_out, labels_out, count_dev,
                 fallback_dev);
    FRCNN_LAUNCH(mosaic_coeffs_kernel, dim3((unsigned)((rows + 255) / 256), 4), dim3(256), 0, s, d);
    FRCNN_LAUNCH(mosaic_h1_kernel, dim3(gw1, (unsigned)hmax, 4), dim3(256), 0, s, d);
    FRCNN_LAUNCH(mosaic_v1_kernel, dim3(gw1, (unsigned)H1max, 4), dim3(256), 0, s, d);
    FRCNN_LAUNCH(mosaic_h2_kernel, dim3(gs, (unsigned)H1max, 4), dim3(256), 0, s, d);
    FRCNN_LAUNCH(mosaic_v2_kernel, dim3(gs, (unsigned)size, 4), dim3(256), 0, s, d, canvas);
    FRCNN_CHECK_LAUNCH("mosaic kernels");
    return FRCNN_OK;
}
