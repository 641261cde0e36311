// coco_eval.hip -- the COCO detection protocol (bbox, useCats = 1) that the reference's test loop scores with (test.py:60-88, 124-128:
// CocoEvaluator.update / accumulate / summarize of evaluation/coco_eval.py, i.e. pycocotools' COCOeval.evaluateImg and accumulate with
// maskUtils.iou on boxes) on the device, fed by ops.Detections with no host sync: one launch per frame, one launch per test set.
//
//  coco_update_kernel : one frame, one workgroup per category.  Every workgroup scans the frame's labels (detections may come in any
//      order), packs the (orderable(score) << 32 | ~position) keys of its category into its segment of the workspace, takes the
//      max_det largest (a radix select over the segment when there are more), ranks them (score descending, position ascending) and
//      forms their pixel xywh boxes in fp32 as test.py:70-71 and convert_to_xywh do, widened to float64.  The category's ground truths
//      are compacted in their original order.  The float64 IoUs (maskUtils.iou's operation order, crowd: union = detection area) are
//      computed by the whole workgroup into an LDS tile of as many detections as fit; then one wave walks the tile with one lane per
//      (area range, threshold) chain, detections in rank order.  evaluateImg's walk over the ground truths sorted non-ignored first is
//      two passes in original order: the non-ignored ones, then -- only when the first pass matched nothing -- the ignored ones; matched
//      non-crowd ground truths are skipped, >= keeps the later of equal IoUs.  Each lane keeps its chain's gtm bits in LDS.  One atomic
//      add per workgroup reserves the category's slots in the record store; a record is (score, label, image_id, rank, one flag word
//      per area range with 2 bits per threshold: TP = matched and not ignored, FP = unmatched and not ignored, IGNORED = the rest).
//      npig[k][a] += the frame's non-ignored ground truths.  No scratch has to be zero between calls.
//  coco_accumulate_kernel : one workgroup per (category, area range) over the records in the order (label ascending, score descending,
//      image_id ascending, rank ascending), for each of the 3 maxDets and each threshold: the scan of eval_dev.h for the cumulative
//      (tp, fp) over the records of rank < M, pr = tp / (fp + tp + 2^-52) stored at the true positives (between them pr only falls
//      and recall does not move, so the envelope and searchsorted(rc, recThr, 'left') need nothing else; position 0 without a true
//      positive holds 0), a right-to-left running maximum as a second scan, and one lane per recall threshold that bisects for the
//      first true positive k with k / npig >= recThr.  The float64 operations of accumulate and no others.
//
// Not built: the segm and keypoints IoU types.  useCats = 0 (every category pooled) is coco_eval_pooled.hip, which feeds the same record store
// and coco_accumulate_kernel with K = 1.
//
// The limits (EVAL_MAX_*, EVAL_THREADS, eval_supported), the error bits of a frame, eval_lower_bound and the (tp, fp) scan are those of
// eval_dev.h, shared with eval.hip.
#include "frcnn_common.h"
#include "frcnn_layout.h"
#include "eval_dev.h"
FRCNN_LAYOUT_STAMP(coco_eval);

#define COCO_MAX_R 256
#define COCO_A 4                       // area ranges: all, small, medium, large
#define COCO_MAX_DET 100               // the per-image cut (maxDets[-1])
#define COCO_TILE 4096                 // IoUs (float64) held in LDS at a time: >= 4 detections x EVAL_MAX_G ground truths
#define COCO_CROWD_BIT 4               // s_gflag: bits 0 .. 3 = ignored in area range a, bit 4 = crowd

// workspace: the packed keys of the frame's detections, one segment per category (any content; nothing must be zero)
struct CocoWs { u64 *keys; size_t total; };

static CocoWs coco_ws_layout(int64_t D, void *workspace)
{
    CocoWs w;
    WsCarver c = WsCarver::any_base(workspace);
    w.keys = c.get<u64>((size_t)D);
    w.total = c.bytes();
    return w;
}

size_t frcnn_ws_coco_eval(int64_t D, int64_t G) { return eval_supported(D, G) ? coco_ws_layout(D, nullptr).total : 0; }

__device__ __forceinline__ bool coco_outside(double area, int a)
{
    const double lo = a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0);           // [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10]
    const double hi = a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10);
    return area < lo || area > hi;
}

__global__ __launch_bounds__(EVAL_THREADS) void coco_update_kernel(
    const float4 *__restrict__ boxes, const int32_t *__restrict__ labels, const float *__restrict__ scores, const int32_t *__restrict__ count_dev,
    int D, const double *__restrict__ gt_boxes, const double *__restrict__ gt_area, const int32_t *__restrict__ gt_labels,
    const uint8_t *__restrict__ gt_crowd, const int32_t *__restrict__ n_gt_dev, int G, const int32_t *__restrict__ frame,
    const double *__restrict__ thr_dev, int T, int max_det, u64 *__restrict__ npig, float *__restrict__ rec_score, int32_t *__restrict__ rec_label,
    int32_t *__restrict__ rec_image, int32_t *__restrict__ rec_rank, uint32_t *__restrict__ rec_flags, long long rec_cap, u64 *__restrict__ cursor,
    int32_t *__restrict__ err, u64 *__restrict__ ws_keys)
{
    __shared__ double s_iou[COCO_TILE];
    __shared__ uint32_t s_gtm[EVAL_MAX_G / 32][64];             // [word][chain]: a lane's words lie in its own bank
    __shared__ int32_t s_gidx[EVAL_MAX_G];
    __shared__ uint8_t s_gflag[EVAL_MAX_G];
    __shared__ u64 s_key[COCO_MAX_DET], s_sorted[COCO_MAX_DET];
    __shared__ double s_dx[COCO_MAX_DET], s_dy[COCO_MAX_DET], s_dxe[COCO_MAX_DET], s_dye[COCO_MAX_DET], s_dwh[COCO_MAX_DET];
    __shared__ uint32_t s_flags[COCO_MAX_DET][COCO_A];
    __shared__ uint8_t s_dout[COCO_MAX_DET];                    // bit a: the detection's area lies outside range a
    __shared__ double s_thr[EVAL_MAX_T];
    __shared__ int s_hist[256];
    __shared__ int s_m, s_off, s_bad, s_fill, s_sel, s_rem;
    __shared__ int s_wcnt[EVAL_THREADS / 64];
    __shared__ u64 s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = blockIdx.x, nc = (int)gridDim.x;
    const int cnt_raw = *count_dev, ng_raw = *n_gt_dev;
    int e = eval_frame_error(cnt_raw, D, ng_raw, G);
    const int n = e ? 0 : cnt_raw;
    const int ng = e ? 0 : (ng_raw < 0 ? 0 : ng_raw);
    if (tid == 0) { s_m = 0; s_off = 0; s_bad = 0; s_fill = 0; }
    if (tid < T) s_thr[tid] = thr_dev[tid];
    __syncthreads();
    // ---- the category's detections: how many, and where its segment of the workspace begins
    {
        int m_loc = 0, off_loc = 0, bad = 0;
        for (int i = tid; i < n; i += EVAL_THREADS) {
            const int l = labels[i];
            if (l < 0 || l >= nc) bad = 1;
            else { m_loc += l == k; off_loc += l < k; }
        }
        for (int g = tid; g < ng; g += EVAL_THREADS) {
            const int l = gt_labels[g];
            if (l < 0 || l >= nc) bad = 1;
        }
        if (m_loc) atomicAdd(&s_m, m_loc);
        if (off_loc) atomicAdd(&s_off, off_loc);
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) e |= EVAL_ERR_LABEL_RANGE;
    // a frame that reports an error is not recorded at all (eval_dev.h)
    if (e) {
        if (k == 0 && tid == 0) atomicOr(err, e);
        return;
    }
    const int m = s_m, off = s_off;
    // ---- the category's ground truths, in their original order
    int mk = 0;
    for (int c0 = 0; c0 < ng; c0 += EVAL_THREADS) {
        const int g = c0 + tid;
        const bool mine = g < ng && gt_labels[g] == k;
        const u64 mask = __ballot(mine);
        if (lane == 0) s_wcnt[wv] = __popcll(mask);
        __syncthreads();
        int base = mk, tot = 0;
        for (int w = 0; w < EVAL_THREADS / 64; ++w) {
            if (w < wv) base += s_wcnt[w];
            tot += s_wcnt[w];
        }
        if (mine) {
            const int j = base + __popcll(mask & ((1ull << lane) - 1ull));
            const bool crowd = gt_crowd[g] != 0;
            const double ar = gt_area[g];
            uint32_t f = crowd ? (1u << COCO_CROWD_BIT) | 15u : 0u;                         // gtIg = iscrowd or area outside the range
            for (int a = 0; a < COCO_A; ++a)
                if (coco_outside(ar, a)) f |= 1u << a;
            s_gidx[j] = g;
            s_gflag[j] = (uint8_t)f;
        }
        mk += tot;
        __syncthreads();
    }
    if (m == 0 && mk == 0) return;                                                          // the pair contributes nothing
    if (tid < COCO_A) {
        int c = 0;
        for (int j = 0; j < mk; ++j) c += !((s_gflag[j] >> tid) & 1u);
        if (c) atomicAdd(&npig[(size_t)k * COCO_A + tid], (u64)c);
    }
    if (m == 0) return;
    // ---- the max_det first detections of the category in (score descending, position ascending)
    const int nd = m < max_det ? m : max_det;
    u64 *seg = ws_keys + off;                                                               // off + m <= n <= D
    for (int i = tid; i < n; i += EVAL_THREADS)
        if (labels[i] == k) {
            const int slot = atomicAdd(&s_fill, 1);
            if (slot < m) seg[slot] = ((u64)eval_orderable(scores[i]) << 32) | (uint32_t)~(uint32_t)i;     // unique per detection
        }
    __syncthreads();
    if (m <= max_det) {
        if (tid < m) s_key[tid] = seg[tid];
    } else {
        // radix select, 8 bits at a time from the top: `prefix` becomes the nd-th largest key
        u64 prefix = 0;
        int remaining = nd;
        for (int shift = 56; shift >= 0; shift -= 8) {
            s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < m; i += EVAL_THREADS) {
                const u64 key = seg[i];
                if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255ull)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int c = 0, d = 255;
                for (; d > 0; --d) {
                    if (c + s_hist[d] >= remaining) break;
                    c += s_hist[d];
                }
                s_sel = d;
                s_rem = remaining - c;
            }
            __syncthreads();
            prefix = (prefix << 8) | (u64)s_sel;
            remaining = s_rem;
        }
        if (tid == 0) s_fill = 0;
        __syncthreads();
        for (int i = tid; i < m; i += EVAL_THREADS) {
            const u64 key = seg[i];
            if (key >= prefix) {
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < nd) s_key[slot] = key;
            }
        }
    }
    __syncthreads();
    if (tid < nd) {
        const u64 key = s_key[tid];
        int r = 0;
        for (int j = 0; j < nd; ++j) r += s_key[j] > key;
        s_sorted[r] = key;
    }
    for (int i = tid; i < (EVAL_MAX_G / 32) * 64; i += EVAL_THREADS) (&s_gtm[0][0])[i] = 0u;
    __syncthreads();
    if (tid < nd) {
        const float4 b = boxes[(uint32_t)~(uint32_t)s_sorted[tid]];
        const float fw = (float)frame[0], fh = (float)frame[1];
        const float X1 = b.x * fw, Y1 = b.y * fh, X2 = b.z * fw, Y2 = b.w * fh;           // test.py:70-71, in fp32
        const float Wf = X2 - X1, Hf = Y2 - Y1;                                             // convert_to_xywh, in fp32
        const double dx = (double)X1, dy = (double)Y1, dw = (double)Wf, dh = (double)Hf;    // .tolist()
        const double area = dw * dh;
        s_dx[tid] = dx; s_dy[tid] = dy; s_dxe[tid] = dx + dw; s_dye[tid] = dy + dh; s_dwh[tid] = area;
        uint32_t o = 0;
        for (int a = 0; a < COCO_A; ++a) {
            if (coco_outside(area, a)) o |= 1u << a;
            s_flags[tid][a] = 0u;
        }
        s_dout[tid] = (uint8_t)o;
    }
    __syncthreads();
    // ---- matching: tiles of `dc` detections x mk ground truths
    const int dc = mk > 0 ? (COCO_TILE / mk < nd ? COCO_TILE / mk : nd) : nd;
    for (int d0 = 0; d0 < nd; d0 += dc) {
        const int cn = nd - d0 < dc ? nd - d0 : dc;
        for (int p = tid; p < cn * mk; p += EVAL_THREADS) {
            const int d = d0 + p / mk, j = p % mk, g = s_gidx[j];
            const double gx = gt_boxes[4 * g], gy = gt_boxes[4 * g + 1], gw = gt_boxes[4 * g + 2], gh = gt_boxes[4 * g + 3];
            double iou = 0.0;
            const double w = fmin(s_dxe[d], gx + gw) - fmax(s_dx[d], gx);
            if (!(w <= 0.0)) {
                const double h = fmin(s_dye[d], gy + gh) - fmax(s_dy[d], gy);
                if (!(h <= 0.0)) {
                    const double i = w * h;
                    const double u = ((s_gflag[j] >> COCO_CROWD_BIT) & 1u) ? s_dwh[d] : s_dwh[d] + gw * gh - i;
                    iou = i / u;
                }
            }
            s_iou[p] = iou;
        }
        __syncthreads();
        if (wv == 0 && lane < COCO_A * T) {
            const int a = lane / T, t = lane % T;
            const double best0 = s_thr[t] < 1.0 - 1e-10 ? s_thr[t] : 1.0 - 1e-10;           // min([t, 1 - 1e-10])
            for (int d = d0; d < d0 + cn; ++d) {
                const double *row = s_iou + (size_t)(d - d0) * mk;
                double best = best0;
                int mm = -1;
                for (uint32_t pass = 0; pass < 2; ++pass) {
                    const bool walking = pass == 0 || mm < 0;                               // the break: a non-ignored match ends the walk
                    if (!__any(walking)) break;
                    for (int j = 0; j < mk; ++j) {
                        const uint32_t f = s_gflag[j];
                        if (!walking || ((f >> a) & 1u) != pass) continue;
                        if (((s_gtm[j >> 5][lane] >> (j & 31)) & 1u) && !((f >> COCO_CROWD_BIT) & 1u)) continue;
                        const double v = row[j];
                        if (v < best) continue;
                        best = v;
                        mm = j;
                    }
                }
                uint32_t code;
                if (mm >= 0) {
                    s_gtm[mm >> 5][lane] |= 1u << (mm & 31);
                    code = ((s_gflag[mm] >> a) & 1u) ? FRCNN_EVAL_IGNORED : FRCNN_EVAL_TP;
                } else {
                    code = ((s_dout[d] >> a) & 1u) ? FRCNN_EVAL_IGNORED : FRCNN_EVAL_FP;
                }
                atomicOr(&s_flags[d][a], code << (2 * t));
            }
        }
        __syncthreads();
    }
    // ---- the records
    if (tid == 0) s_base = atomicAdd(cursor, (u64)nd);                                      // a full store keeps counting: summarize() reports the loss
    __syncthreads();
    if (tid < nd) {
        const u64 slot = s_base + (u64)tid;
        if (slot < (u64)rec_cap) {
            rec_score[slot] = scores[(uint32_t)~(uint32_t)s_sorted[tid]];
            rec_label[slot] = k;
            rec_image[slot] = frame[2];
            rec_rank[slot] = tid;
            for (int a = 0; a < COCO_A; ++a) rec_flags[slot * COCO_A + a] = s_flags[tid][a];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// accumulate
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_THREADS) void coco_accumulate_kernel(
    const int32_t *__restrict__ labels, const int32_t *__restrict__ ranks, const uint32_t *__restrict__ flags, const u64 *__restrict__ n_dev,
    long long cap, const u64 *__restrict__ npig, const double *__restrict__ rec_thr, int R, int T, int K, int md0, int md1, int md2,
    double *__restrict__ precision, double *__restrict__ recall, double *__restrict__ prec_ws)
{
    __shared__ u64 s_wave[EVAL_THREADS / 64];
    __shared__ u64 s_carry;
    __shared__ double s_wmax[EVAL_THREADS / 64];
    __shared__ double s_cmax;
    const int k = blockIdx.x / COCO_A, a = blockIdx.x % COCO_A;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 np = npig[(size_t)k * COCO_A + a];
    if (np == 0) {                                                                          // the cells stay at -1
        for (int i = tid; i < 3 * T * R; i += EVAL_THREADS) {
            const int mi = i % 3, r = (i / 3) % R, t = i / (3 * R);
            precision[((((size_t)t * R + r) * K + k) * COCO_A + a) * 3 + mi] = -1.0;
        }
        for (int i = tid; i < 3 * T; i += EVAL_THREADS) recall[(((size_t)(i / 3) * K + k) * COCO_A + a) * 3 + i % 3] = -1.0;
        return;
    }
    const u64 n_raw = *n_dev;
    const long long n = n_raw < (u64)cap ? (long long)n_raw : cap;
    const long long lo = eval_lower_bound(labels, n, k), hi = eval_lower_bound(labels, n, k + 1);
    const double dn = (double)np;
    double *pk = prec_ws + (size_t)a * (size_t)cap + lo;          // this (category, area range)'s own segment: at most hi - lo true positives
    for (int mi = 0; mi < 3; ++mi) {
        const int M = mi == 0 ? md0 : (mi == 1 ? md1 : md2);
        for (int t = 0; t < T; ++t) {
            if (tid == 0) { s_carry = 0ull; s_cmax = 0.0; }
            __syncthreads();
            for (long long c0 = lo; c0 < hi; c0 += EVAL_THREADS) {
                const long long i = c0 + tid;
                const uint32_t f = (i < hi && ranks[i] < M) ? (flags[i * COCO_A + a] >> (2 * t)) & 3u : 0u;
                const u64 v = eval_scan_step(f, s_wave, &s_carry);                          // the cumulative (tp, fp) over the records of rank < M
                if (f == FRCNN_EVAL_TP) {
                    const long long tpc = (long long)(v & 0xffffffffull), fpc = (long long)(v >> 32);
                    pk[tpc - 1] = (double)tpc / (((double)fpc + (double)tpc) + 0x1p-52);    // tp / (fp + tp + np.spacing(1))
                }
                eval_scan_carry(v, &s_carry);
            }
            const long long Kt = (long long)(s_carry & 0xffffffffull);
            // pr made non-increasing from the right: a running maximum over the true positives, last to first
            for (long long c0 = 0; c0 < Kt; c0 += EVAL_THREADS) {
                const long long i = Kt - 1 - (c0 + tid);
                double v = i >= 0 ? pk[i] : 0.0;
                for (int o = 1; o < 64; o <<= 1) {
                    const double u = __shfl_up(v, o);
                    if (lane >= o && u > v) v = u;
                }
                if (lane == 63) s_wmax[wv] = v;
                __syncthreads();
                double pre = s_cmax;
                for (int w = 0; w < wv; ++w) pre = s_wmax[w] > pre ? s_wmax[w] : pre;
                if (pre > v) v = pre;
                if (i >= 0) pk[i] = v;
                __syncthreads();
                if (tid == EVAL_THREADS - 1) s_cmax = v;
                __syncthreads();
            }
            __syncthreads();
            // precision at searchsorted(rc, recThr, 'left'): the first true positive kk with kk / npig >= recThr; 0 past the end
            for (int r = tid; r < R; r += EVAL_THREADS) {
                const double thr = rec_thr[r];
                long long a0 = 1, b0 = Kt + 1;
                while (a0 < b0) {
                    const long long mid = (a0 + b0) >> 1;
                    if ((double)mid / dn < thr) a0 = mid + 1; else b0 = mid;
                }
                precision[((((size_t)t * R + r) * K + k) * COCO_A + a) * 3 + mi] = a0 <= Kt ? pk[a0 - 1] : 0.0;
            }
            if (tid == 0) recall[(((size_t)t * K + k) * COCO_A + a) * 3 + mi] = (double)Kt / dn;      // rc[-1], 0 without detections
            __syncthreads();
        }
    }
}

FRCNN_EXPORT int frcnn_coco_eval_update(const float *boxes, const int32_t *labels, const float *scores, const int32_t *count_dev,
                                        int64_t det_capacity, const double *gt_boxes, const double *gt_area, const int32_t *gt_labels,
                                        const uint8_t *gt_iscrowd, const int32_t *n_gt_dev, int64_t gt_capacity, const int32_t *frame_dev,
                                        const double *thresholds_dev, int T, int C, int max_det, int64_t *npig, float *rec_score,
                                        int32_t *rec_label, int32_t *rec_image, int32_t *rec_rank, uint32_t *rec_flags, int64_t record_capacity,
                                        int64_t *cursor, int32_t *error_word, void *workspace, size_t workspace_bytes, void *stream)
{
    if (C < 2 || C > EVAL_MAX_C || T < 1 || T > EVAL_MAX_T || max_det < 1 || max_det > COCO_MAX_DET || !eval_supported(det_capacity, gt_capacity) ||
        det_capacity > (int64_t)(C - 1) * EVAL_MAX_P)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED,
                               "coco_eval_update: C = %d, T = %d, max_det = %d, detection capacity %lld, ground-truth capacity %lld outside "
                               "2 <= C <= %d, 1 <= T <= %d, 1 <= max_det <= %d, 1 <= D <= (C-1) * %d, 1 <= G <= %d", C, T, max_det,
                               (long long)det_capacity, (long long)gt_capacity, EVAL_MAX_C, EVAL_MAX_T, COCO_MAX_DET, EVAL_MAX_P, EVAL_MAX_G);
    FRCNN_REQUIRE(boxes && labels && scores && count_dev && gt_boxes && gt_area && gt_labels && gt_iscrowd && n_gt_dev && frame_dev && thresholds_dev &&
                  npig && rec_score && rec_label && rec_image && rec_rank && rec_flags && cursor && error_word && workspace,
                  "coco_eval_update: NULL pointer");
    FRCNN_REQUIRE(record_capacity >= 1, "coco_eval_update: record_capacity must be >= 1");
    FRCNN_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt_boxes & 7) == 0 && ((uintptr_t)gt_area & 7) == 0,
                  "coco_eval_update: boxes must be 16-byte aligned, gt_boxes and gt_area 8-byte aligned");
    const CocoWs w = coco_ws_layout(det_capacity, workspace);
    FRCNN_REQUIRE_WS("coco_eval_update", workspace_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(coco_update_kernel, dim3((unsigned)(C - 1)), dim3(EVAL_THREADS), 0, s, (const float4 *)boxes, labels, scores, count_dev,
                 (int)det_capacity, gt_boxes, gt_area, gt_labels, gt_iscrowd, n_gt_dev, (int)gt_capacity, frame_dev, thresholds_dev, T, max_det,
                 (u64 *)npig, rec_score, rec_label, rec_image, rec_rank, rec_flags, (long long)record_capacity, (u64 *)cursor, error_word, w.keys);
    FRCNN_CHECK_LAUNCH("coco_update_kernel");
    return FRCNN_OK;
}

FRCNN_EXPORT int frcnn_coco_eval_accumulate(const int32_t *labels_sorted, const int32_t *ranks_sorted, const uint32_t *flags_sorted,
                                            const int64_t *n_dev, int64_t capacity, const int64_t *npig, const double *rec_thresholds_dev, int R,
                                            int T, int C, int max_det_0, int max_det_1, int max_det_2, double *precision, double *recall,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    if (C < 2 || C > EVAL_MAX_C || T < 1 || T > EVAL_MAX_T || R < 1 || R > COCO_MAX_R)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "coco_eval_accumulate: C = %d, T = %d, R = %d outside 2 <= C <= %d, 1 <= T <= %d, 1 <= R <= %d",
                               C, T, R, EVAL_MAX_C, EVAL_MAX_T, COCO_MAX_R);
    FRCNN_REQUIRE(labels_sorted && ranks_sorted && flags_sorted && n_dev && npig && rec_thresholds_dev && precision && recall && workspace,
                  "coco_eval_accumulate: NULL pointer");
    FRCNN_REQUIRE(capacity >= 1, "coco_eval_accumulate: capacity must be >= 1");
    FRCNN_REQUIRE(max_det_0 >= 1 && max_det_1 >= 1 && max_det_2 >= 1, "coco_eval_accumulate: maxDets must be >= 1");
    WsCarver c = WsCarver::any_base(workspace);
    double *pw = (double *)c.here();                            // one piece, sized to the byte (not rounded up to the carver's 256)
    FRCNN_REQUIRE_WS("coco_eval_accumulate", workspace_bytes, c.bytes() + (size_t)COCO_A * (size_t)capacity * sizeof(double));
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(coco_accumulate_kernel, dim3((unsigned)((C - 1) * COCO_A)), dim3(EVAL_THREADS), 0, s, labels_sorted, ranks_sorted, flags_sorted,
                 (const u64 *)n_dev, (long long)capacity, (const u64 *)npig, rec_thresholds_dev, R, T, C - 1, max_det_0, max_det_1, max_det_2,
                 precision, recall, pw);
    FRCNN_CHECK_LAUNCH("coco_accumulate_kernel");
    return FRCNN_OK;
}
