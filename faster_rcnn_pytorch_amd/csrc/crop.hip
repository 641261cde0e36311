// crop.hip -- the crop of the wired pipeline (new_datasets/transforms.py:16-56; RandomCrop :162-168, RandomSizeCrop :171-180, CenterCrop
// :183-192) for one uint8 HWC frame already in HBM, with the resize in front of it (:76-132) folded in:
//   resize(frame, (H1, W1)) -> crop(region (i, j, ch, cw))      (H1, W1) == (h, w): a plain crop
// This crop ALWAYS crops (unlike datasets/transforms_.py:crop_, which hands back the uncropped frame when no box survives: mosaic.hip), so
// the output shape is the region, which the host knows; only the NUMBER of surviving boxes is device data.  It goes to a device count
// behind fixed-capacity lists, as everywhere in this library.  A fixed number of launches whatever the boxes say, no host read-back:
//   four with a resize:
//     crop_boxes_kernel  : ONE workgroup: resize ratios, shift, min, clamp, area, the keep rule, and the compaction of boxes / labels /
//                          area / iscrowd in input order, 256 rows at a time (ballot + popcount inside a wave, four wave totals through
//                          LDS, a running base across chunks, as mosaic_boxes_kernel); zeros behind the live rows, the count
//     crop_coeffs_kernel : Pillow's windows of the region's cw columns and ch rows only
//     crop_h_kernel      : horizontal pass, the region's columns on just the source rows the region's vertical windows reach -> a real
//                          uint8 intermediate, as Pillow has between its passes
//     crop_v_kernel      : vertical pass -> the [ch, cw, 3] image: the bytes of F.resize followed by F.crop on a PIL image
//   two for a plain crop ((H1, W1) == (h, w); Pillow returns a copy for an equal size):
//     crop_boxes_kernel, crop_copy_kernel (the region's bytes).  The resampler would give the same bytes (at scale 1 a window has one tap
//     of weight 1); the copy is just cheaper.
// Which of the two runs depends on host integers alone.
// A region that is not inside the resized frame is REFUSED: PIL's Image.crop would pad it with black, and no recipe of the reference
// draws one (get_params and CenterCrop on a frame no smaller than the crop stay inside).  Byte gathers through short windows: latency
// and launch bound at these sizes, not bandwidth.  Box arithmetic is the reference's, operation for operation, in binary32
// (-ffp-contract=off).
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
FRCNN_LAYOUT_STAMP(crop);
#include "resample_dev.h"

struct CropBoxes {
    const float4 *boxes; const int64_t *labels, *iscrowd;       // iscrowd may be NULL (then iscrowd_out is too)
    float4 *boxes_out; int64_t *labels_out, *iscrowd_out; float *area_out;      // area_out may be NULL
    const int32_t *count_in;                                     // NULL: all n rows are live
    int32_t *count_out;
    int n;
    float rw, rh;                                                // transforms.py:111: float(new) / float(old), formed in double
    float fi, fj, fch, fcw;
};

__global__ __launch_bounds__(256) void crop_boxes_kernel(CropBoxes d)
{
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int live = d.n;
    if (d.count_in) { const int c = *d.count_in; live = c < 0 ? 0 : (c < d.n ? c : d.n); }
    int base = 0;                                                     // live rows so far: the same in every thread
    for (int c0 = 0; c0 < live; c0 += 256) {                          // uniform trip count: every thread reaches both barriers
        const int i = c0 + tid;
        bool keep = false;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < live) {
            const float4 b = d.boxes[i];
            const float sx1 = b.x * d.rw, sy1 = b.y * d.rh, sx2 = b.z * d.rw, sy2 = b.w * d.rh;                           // :117
            float x1 = tmin(sx1 - d.fj, d.fcw), y1 = tmin(sy1 - d.fi, d.fch), x2 = tmin(sx2 - d.fj, d.fcw), y2 = tmin(sy2 - d.fi, d.fch);   // :30-31
            x1 = x1 < 0.0f ? 0.0f : x1; y1 = y1 < 0.0f ? 0.0f : y1; x2 = x2 < 0.0f ? 0.0f : x2; y2 = y2 < 0.0f ? 0.0f : y2;   // :32 (NaN stays)
            o = make_float4(x1, y1, x2, y2);
            keep = x2 > x1 && y2 > y1;                                                                                   // :48-49 (NaN compares false)
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wave; ++q) off += s_wave[q];
        if (keep) {
            off += __popcll(m & ((1ull << lane) - 1ull));
            d.boxes_out[off] = o;
            d.labels_out[off] = d.labels[i];
            if (d.area_out) d.area_out[off] = (o.z - o.x) * (o.w - o.y);                                                  // :33
            if (d.iscrowd_out) d.iscrowd_out[off] = d.iscrowd[i];
        }
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    for (int i = base + tid; i < d.n; i += 256) {
        d.boxes_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); d.labels_out[i] = 0;
        if (d.area_out) d.area_out[i] = 0.0f;
        if (d.iscrowd_out) d.iscrowd_out[i] = 0;
    }
    if (tid == 0) *d.count_out = base;
}

struct CropImg {
    const uint8_t *src; uint8_t *out;
    int h, w, H1, W1, i, j, ch, cw;
    int ksx, ksy, rows_cap;               // table strides; rows of tmp: no fewer than the source rows the region's vertical windows span
    int32_t *bx, *by, *kx, *ky;           // [cw, 2], [ch, 2], [cw, ksx], [ch, ksy]: the region's columns and rows, region-relative index
    uint8_t *tmp;                         // [rows_cap, cw, 3]: row 0 is source row by[0]
};

__global__ __launch_bounds__(256) void crop_coeffs_kernel(CropImg d)
{
    int q = blockIdx.x * 256 + threadIdx.x;
    if (q < d.cw) { rs_coeffs_at(d.j + q, d.w, d.W1, d.ksx, d.bx + 2 * q, d.kx + (size_t)q * d.ksx); return; }
    q -= d.cw;
    if (q < d.ch) rs_coeffs_at(d.i + q, d.h, d.H1, d.ksy, d.by + 2 * q, d.ky + (size_t)q * d.ksy);
}

// horizontal pass: the region's columns, on the source rows [ylo, yhi) its rows' windows reach (windows start in non-decreasing order)
__global__ __launch_bounds__(256) void crop_h_kernel(CropImg d)
{
    const int x = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    const int ylo = d.by[0], yhi = d.by[2 * (d.ch - 1)] + d.by[2 * (d.ch - 1) + 1];
    const int y = ylo + r;
    if (x >= d.cw || r >= d.rows_cap || y >= yhi || y < 0 || y >= d.h) return;
    const int xmin = d.bx[2 * x], n = d.bx[2 * x + 1];
    if (xmin < 0 || n < 0 || n > d.ksx || xmin + n > d.w) return;           // never taken: rs_coeffs_at clips the window to the frame
    uint8_t px[3];
    rs_window_rgb(d.src + ((size_t)y * d.w + xmin) * 3, 3, n, d.kx + (size_t)x * d.ksx, px);
    uint8_t *o = d.tmp + ((size_t)r * d.cw + x) * 3;
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
}

__global__ __launch_bounds__(256) void crop_v_kernel(CropImg d)
{
    const int x = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
    if (x >= d.cw || yy >= d.ch) return;
    const int ylo = d.by[0];
    const int r0 = d.by[2 * yy] - ylo, n = d.by[2 * yy + 1];
    if (r0 < 0 || n < 0 || n > d.ksy || r0 + n > d.rows_cap) return;        // never taken: rows_cap bounds the span (crop_rows_cap)
    uint8_t px[3];
    rs_window_rgb(d.tmp + ((size_t)r0 * d.cw + x) * 3, (ptrdiff_t)d.cw * 3, n, d.ky + (size_t)yy * d.ksy, px);
    uint8_t *o = d.out + ((size_t)yy * d.cw + x) * 3;
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
}

// plain crop: one thread per byte of a region row
__global__ __launch_bounds__(256) void crop_copy_kernel(CropImg d)
{
    const int b = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
    if (b >= d.cw * 3 || yy >= d.ch) return;
    d.out[(size_t)yy * d.cw * 3 + b] = d.src[((size_t)(d.i + yy) * d.w + d.j) * 3 + b];
}

// An upper bound of the source rows the vertical windows of ch consecutive output rows span.  Window r starts no earlier than
// center_r - support + 0.5 - 1 and ends before center_r + support + 0.5, and center_r advances by scale: the span of the first start to
// the last end is below (ch - 1) * scale + 2 * support + 1.  One more row of slack; never more than the frame has.
static int crop_rows_cap(int h, int H1, int ch)
{
    const double scale = (double)h / (double)H1, support = scale < 1.0 ? 1.0 : scale;
    const double span = (double)(ch - 1) * scale + 2.0 * support + 2.0;
    return span >= (double)h ? h : (int)span;
}

static bool crop_shapes_ok(int h, int w, int H1, int W1, int ch, int cw)
{
    const int lim = 1 << 15;
    return h >= 1 && w >= 1 && H1 >= 1 && W1 >= 1 && ch >= 1 && cw >= 1 && h < lim && w < lim && H1 < lim && W1 < lim && ch <= H1 && cw <= W1;
}

static size_t crop_ws_layout(void *base, CropImg *d)
{
    size_t o = 0;
    auto take = [&](size_t bytes) { void *q = base ? (char *)base + o : nullptr; o += align_up(bytes, 256); return q; };
    d->ksx = rs_ksize_host(d->w, d->W1); d->ksy = rs_ksize_host(d->h, d->H1);
    d->rows_cap = crop_rows_cap(d->h, d->H1, d->ch);
    d->bx = (int32_t *)take((size_t)d->cw * 8); d->by = (int32_t *)take((size_t)d->ch * 8);
    d->kx = (int32_t *)take((size_t)d->cw * d->ksx * 4); d->ky = (int32_t *)take((size_t)d->ch * d->ksy * 4);
    d->tmp = (uint8_t *)take((size_t)d->rows_cap * d->cw * 3);
    return o;
}

FRCNN_EXPORT size_t frcnn_resize_crop_workspace(int h, int w, int H1, int W1, int ch, int cw)
{
    if (!crop_shapes_ok(h, w, H1, W1, ch, cw)) return 0;
    CropImg d = {};
    d.h = h; d.w = w; d.H1 = H1; d.W1 = W1; d.ch = ch; d.cw = cw;
    return crop_ws_layout(nullptr, &d);
}

static bool crop_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

FRCNN_EXPORT int frcnn_resize_crop(const uint8_t *src_hwc, int h, int w, int H1, int W1, int i, int j, int ch, int cw, const float *boxes,
                                   const int64_t *labels, const int64_t *iscrowd, int64_t n, const int32_t *count_in_dev, uint8_t *out_hwc,
                                   float *boxes_out, int64_t *labels_out, float *area_out, int64_t *iscrowd_out, int32_t *count_dev,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(n >= 0 && n <= INT32_MAX, "resize_crop: n = %lld (must be 0 .. 2^31 - 1)", (long long)n);
    FRCNN_REQUIRE(h >= 1 && w >= 1 && H1 >= 1 && W1 >= 1 && h < (1 << 15) && w < (1 << 15) && H1 < (1 << 15) && W1 < (1 << 15),
                  "resize_crop: bad shape %d x %d -> %d x %d (every side must be 1 .. 32767)", h, w, H1, W1);
    FRCNN_REQUIRE(ch >= 1 && cw >= 1, "resize_crop: region has h = %d, w = %d (both must be >= 1)", ch, cw);
    FRCNN_REQUIRE(i >= 0 && j >= 0 && ch <= H1 - i && cw <= W1 - j,
                  "resize_crop: region (i %d, j %d, h %d, w %d) is outside the resized frame %d x %d (PIL would pad it with black; not supported)", i,
                  j, ch, cw, H1, W1);
    FRCNN_REQUIRE(src_hwc && out_hwc && count_dev && workspace, "resize_crop: NULL pointer");
    FRCNN_REQUIRE(n == 0 || (boxes && labels && boxes_out && labels_out), "resize_crop: NULL box / label pointer with %lld boxes", (long long)n);
    FRCNN_REQUIRE((iscrowd == nullptr) == (iscrowd_out == nullptr) || n == 0, "resize_crop: iscrowd and iscrowd_out must both be given or both be NULL");
    FRCNN_REQUIRE(((uintptr_t)boxes | (uintptr_t)boxes_out) % 16 == 0, "resize_crop: boxes and boxes_out must be 16-byte aligned");
    FRCNN_REQUIRE(!crop_overlap(boxes, (size_t)n * 16, boxes_out, (size_t)n * 16) && !crop_overlap(labels, (size_t)n * 8, labels_out, (size_t)n * 8) &&
                      !crop_overlap(iscrowd, (size_t)n * 8, iscrowd_out, (size_t)n * 8),
                  "resize_crop: an output list overlaps its input");
    FRCNN_REQUIRE(!crop_overlap(src_hwc, (size_t)h * w * 3, out_hwc, (size_t)ch * cw * 3), "resize_crop: the output image overlaps the source");
    CropImg d = {};
    d.src = src_hwc; d.out = out_hwc; d.h = h; d.w = w; d.H1 = H1; d.W1 = W1; d.i = i; d.j = j; d.ch = ch; d.cw = cw;
    const size_t need = crop_ws_layout(workspace, &d);
    if (workspace_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "resize_crop: workspace %zu < %zu", workspace_bytes, need);
    CropBoxes b = {};
    b.boxes = (const float4 *)boxes; b.labels = labels; b.iscrowd = n ? iscrowd : nullptr;
    b.boxes_out = (float4 *)boxes_out; b.labels_out = labels_out; b.iscrowd_out = n ? iscrowd_out : nullptr; b.area_out = n ? area_out : nullptr;
    b.count_in = count_in_dev; b.count_out = count_dev; b.n = (int)n;
    b.rw = (float)((double)W1 / (double)w); b.rh = (float)((double)H1 / (double)h);
    b.fi = (float)i; b.fj = (float)j; b.fch = (float)ch; b.fcw = (float)cw;
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(crop_boxes_kernel, dim3(1), dim3(256), 0, s, b);
    if (H1 == h && W1 == w) {
        FRCNN_LAUNCH(crop_copy_kernel, dim3((unsigned)((cw * 3 + 255) / 256), (unsigned)ch), dim3(256), 0, s, d);
    } else {
        const unsigned gx = (unsigned)((cw + 255) / 256);
        FRCNN_LAUNCH(crop_coeffs_kernel, dim3((unsigned)((cw + ch + 255) / 256)), dim3(256), 0, s, d);
        FRCNN_LAUNCH(crop_h_kernel, dim3(gx, (unsigned)d.rows_cap), dim3(256), 0, s, d);
        FRCNN_LAUNCH(crop_v_kernel, dim3(gx, (unsigned)ch), dim3(256), 0, s, d);
    }
    FRCNN_CHECK_LAUNCH("resize_crop kernels");
    return FRCNN_OK;
}
