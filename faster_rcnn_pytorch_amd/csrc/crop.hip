// crop.hip -- the crop of the wired pipeline (new_datasets/transforms.py:16-56; RandomCrop :162-168, RandomSizeCrop :171-180, CenterCrop
// :183-192) for one uint8 HWC frame already in HBM, with the resize in front of it (:76-132) folded in:
//   resize(frame, (H1, W1)) -> crop(region (i, j, ch, cw))      (H1, W1) == (h, w): a plain crop
// This crop ALWAYS crops (unlike datasets/transforms_.py:crop_, which hands back the uncropped frame when no box survives: mosaic.hip), so
// the output shape is the region, which the host knows; only the NUMBER of surviving boxes is device data.  It goes to a device count
// behind fixed-capacity lists, as everywhere in this library.  A fixed number of launches whatever the boxes say, no host read-back:
//   four with a resize:
//     crop_boxes_kernel  : ONE workgroup: resize ratios, shift, min, clamp, area, the keep rule, and the compaction of boxes / labels /
//                          area / iscrowd in input order, 256 rows at a time (in_compact_slot); zeros behind the live rows, the
//                          count
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
#include "input_dev.h"

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
    const int tid = threadIdx.x;
    int live = d.n;
    if (d.count_in) { const int c = *d.count_in; live = c < 0 ? 0 : (c < d.n ? c : d.n); }
    int base = 0;                                                     // live rows so far: the same in every thread
    for (int c0 = 0; c0 < live; c0 += 256) {                          // uniform trip count: every thread makes every in_compact_slot call
        const int i = c0 + tid;
        bool keep = false;
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < live) {
            const float4 b = d.boxes[i];
            keep = in_clip_box(make_float4(b.x * d.rw, b.y * d.rh, b.z * d.rw, b.w * d.rh), d.fi, d.fj, d.fch, d.fcw, &o);      // :117, :30-32, :48-49
        }
        const int off = in_compact_slot(keep, base, s_wave);
        if (keep) {
            d.boxes_out[off] = o;
            d.labels_out[off] = d.labels[i];
            if (d.area_out) d.area_out[off] = (o.z - o.x) * (o.w - o.y);                                                  // :33
            if (d.iscrowd_out) d.iscrowd_out[off] = d.iscrowd[i];
        }
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
    int rows_cap;                         // rows of tmp: no fewer than the source rows the region's vertical windows span
    RsAxis x, y;                          // cw and ch rows: the region's columns and rows, region-relative index
    uint8_t *tmp;                         // [rows_cap, cw, 3]: row 0 is source row y.b[0]
};

__global__ __launch_bounds__(256) void crop_coeffs_kernel(CropImg d)
{
    int q = blockIdx.x * 256 + threadIdx.x;
    if (q < d.cw) { rs_axis_coeffs(d.x, q, d.j + q, d.w, d.W1); return; }
    q -= d.cw;
    if (q < d.ch) rs_axis_coeffs(d.y, q, d.i + q, d.h, d.H1);
}

// horizontal pass: the region's columns, on the source rows [ylo, yhi) its rows' windows reach (windows start in non-decreasing order)
__global__ __launch_bounds__(256) void crop_h_kernel(CropImg d)
{
    const int x = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    const int ylo = d.y.b[0], yhi = d.y.b[2 * (d.ch - 1)] + d.y.b[2 * (d.ch - 1) + 1];
    const int y = ylo + r;
    if (x >= d.cw || r >= d.rows_cap || y >= yhi || y < 0 || y >= d.h) return;
    const int xmin = d.x.b[2 * x], n = d.x.b[2 * x + 1];
    if (xmin < 0 || n < 0 || n > d.x.ks || xmin + n > d.w) return;          // never taken: rs_coeffs_at clips the window to the frame
    rs_pass_px(d.x, x, d.src + (size_t)y * d.w * 3, 3, 0, d.tmp + ((size_t)r * d.cw + x) * 3);
}

__global__ __launch_bounds__(256) void crop_v_kernel(CropImg d)
{
    const int x = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
    if (x >= d.cw || yy >= d.ch) return;
    const int ylo = d.y.b[0];
    const int r0 = d.y.b[2 * yy] - ylo, n = d.y.b[2 * yy + 1];
    if (r0 < 0 || n < 0 || n > d.y.ks || r0 + n > d.rows_cap) return;       // never taken: rows_cap bounds the span (crop_rows_cap)
    rs_pass_px(d.y, yy, d.tmp + (size_t)x * 3, (ptrdiff_t)d.cw * 3, ylo, d.out + ((size_t)yy * d.cw + x) * 3);      // tmp's row 0 is source row ylo
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
    return in_side_ok(h) && in_side_ok(w) && in_side_ok(H1) && in_side_ok(W1) && ch >= 1 && cw >= 1 && ch <= H1 && cw <= W1;
}

static size_t crop_ws_layout(void *base, CropImg *d)
{
    WsCarver c(base);
    d->rows_cap = crop_rows_cap(d->h, d->H1, d->ch);
    d->x = rs_axis_take(c, d->w, d->W1, d->cw);
    d->y = rs_axis_take(c, d->h, d->H1, d->ch);
    d->tmp = c.get<uint8_t>((size_t)d->rows_cap * d->cw * 3);
    return c.bytes();
}

FRCNN_EXPORT size_t frcnn_resize_crop_workspace(int h, int w, int H1, int W1, int ch, int cw)
{
    if (!crop_shapes_ok(h, w, H1, W1, ch, cw)) return 0;
    CropImg d = {};
    d.h = h; d.w = w; d.H1 = H1; d.W1 = W1; d.ch = ch; d.cw = cw;
    return crop_ws_layout(nullptr, &d);
}

FRCNN_EXPORT int frcnn_resize_crop(const uint8_t *src_hwc, int h, int w, int H1, int W1, int i, int j, int ch, int cw, const float *boxes,
                                   const int64_t *labels, const int64_t *iscrowd, int64_t n, const int32_t *count_in_dev, uint8_t *out_hwc,
                                   float *boxes_out, int64_t *labels_out, float *area_out, int64_t *iscrowd_out, int32_t *count_dev,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(n >= 0 && n <= INT32_MAX, "resize_crop: n = %lld (must be 0 .. 2^31 - 1)", (long long)n);
    FRCNN_REQUIRE(in_side_ok(h) && in_side_ok(w) && in_side_ok(H1) && in_side_ok(W1),
                  "resize_crop: bad shape %d x %d -> %d x %d (every side must be 1 .. 32767)", h, w, H1, W1);
    FRCNN_REQUIRE(ch >= 1 && cw >= 1, "resize_crop: region has h = %d, w = %d (both must be >= 1)", ch, cw);
    FRCNN_REQUIRE(i >= 0 && j >= 0 && ch <= H1 - i && cw <= W1 - j,
                  "resize_crop: region (i %d, j %d, h %d, w %d) is outside the resized frame %d x %d (PIL would pad it with black; not supported)", i,
                  j, ch, cw, H1, W1);
    FRCNN_REQUIRE(src_hwc && out_hwc && count_dev && workspace, "resize_crop: NULL pointer");
    FRCNN_REQUIRE(n == 0 || (boxes && labels && boxes_out && labels_out), "resize_crop: NULL box / label pointer with %lld boxes", (long long)n);
    FRCNN_REQUIRE((iscrowd == nullptr) == (iscrowd_out == nullptr) || n == 0, "resize_crop: iscrowd and iscrowd_out must both be given or both be NULL");
    FRCNN_REQUIRE(((uintptr_t)boxes | (uintptr_t)boxes_out) % 16 == 0, "resize_crop: boxes and boxes_out must be 16-byte aligned");
    FRCNN_REQUIRE(!in_overlap(boxes, (size_t)n * 16, boxes_out, (size_t)n * 16) && !in_overlap(labels, (size_t)n * 8, labels_out, (size_t)n * 8) &&
                      !in_overlap(iscrowd, (size_t)n * 8, iscrowd_out, (size_t)n * 8),
                  "resize_crop: an output list overlaps its input");
    FRCNN_REQUIRE(!in_overlap(src_hwc, (size_t)h * w * 3, out_hwc, (size_t)ch * cw * 3), "resize_crop: the output image overlaps the source");
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
