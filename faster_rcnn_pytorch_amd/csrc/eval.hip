// eval.hip -- the VOC average-precision protocol of the reference's evaluator (evaluation/voc_eval.py:67-112 save_pred, :115-135 voc_ap,
// :138-225 cal_mAP) on the device, fed by ops.Detections with no host sync: one launch per frame, one launch per test set.
//
//  eval_update_kernel : one frame.  The frame's ground truth staged in LDS as float64 pixel boxes; one lane per detection (grid-stride
//      over at most EVAL_MAX_WG workgroups) turns its normalised fp32 box into pixels as double(box) * double(w or h) (:90-91, exact)
//      and takes the argmax of the devkit's "+1" overlap over the same-class ground truths in float64, in Python's operation order
//      (:170-180: strict >, from -1, so the first ground truth wins a tie; used and difficult ones take part).  The argmax does not
//      depend on the `used` flags and a ground truth belongs to one frame, so the sequential decision of :184-197 is a per-frame
//      question: a detection is the true positive of its match iff it is the FIRST, in (score descending, position ascending), of the
//      frame's detections that share the match and reach the threshold.  "First" is an atomic max on a 64-bit word per
//      (threshold, ground truth) of (orderable(score) << 32 | ~position): unique per detection, hence deterministic.  The workgroup
//      that finishes last (an agent-scope ticket, as in loss.hip) reserves the frame's slots in the record store with ONE atomic add
//      on the device cursor, writes the records (score, label, image_id, position, flags: 2 bits per threshold) and leaves the winner
//      words and the ticket zero for the next call.  Slot order is irrelevant: the defined order (score descending, image_id
//      ascending, position ascending) is restored when the set is summarised.
//  eval_ap_kernel     : one workgroup per class over the records in the defined order.  Recall changes exactly at the true positives
//      and the precision envelope's running maximum is taken at them only (precision falls at every false positive), so the
//      workgroup scans the class's segment for the cumulative (tp, fp) (the scan of eval_dev.h), stores precision k / max(k + fp, eps) of the k-th true positive,
//      and one lane takes the right-to-left maximum and adds (k / npos - (k - 1) / npos) * mpre in ascending k: the same float64
//      operations in the same order as voc_ap.  A class without a countable ground truth reports NaN (the reference does not know it).
//
// Not reproduced: save_pred's `class_num == 20: continue` (:100-103), a FIXME for a background id that never occurs with the 0-based
// labels detect produces.
//
// The limits (EVAL_MAX_*, EVAL_THREADS, eval_supported), the error bits of a frame, eval_lower_bound and the (tp, fp) scan are those of
// eval_dev.h, shared with coco_eval.hip.
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "eval_dev.h"
FRCNN_LAYOUT_STAMP(eval);

#define EVAL_MAX_WG 64

// workspace: ticket (64 bytes) | winner words [EVAL_MAX_T][G] u64 | match [D] i32 | reach [D] u32, each 256-byte aligned.  The ticket
// and the winner words must be ZERO before the first call; the kernel leaves them zero.
struct EvalWs { int32_t *ticket; u64 *win; int32_t *match; uint32_t *reach; size_t total; };

static EvalWs eval_ws_layout(int64_t D, int64_t G, void *workspace)
{
    EvalWs w;
    WsCarver c = WsCarver::any_base(workspace);
    w.ticket = c.get<int32_t>(16);
    w.win = c.get<u64>((size_t)EVAL_MAX_T * (size_t)G);
    w.match = c.get<int32_t>((size_t)D);
    w.reach = c.get<uint32_t>((size_t)D);
    w.total = c.bytes();
    return w;
}

size_t frcnn_ws_eval(int64_t D, int64_t G) { return eval_supported(D, G) ? eval_ws_layout(D, G, nullptr).total : 0; }

// Python's max(a, b) / min(a, b): the first argument unless the second is strictly beyond it (a NaN first argument stays)
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

__global__ __launch_bounds__(EVAL_THREADS) void eval_update_kernel(
    const float4 *__restrict__ boxes, const int32_t *__restrict__ labels, const float *__restrict__ scores, const int32_t *__restrict__ count_dev,
    int D, const float4 *__restrict__ gt_boxes, const int32_t *__restrict__ gt_labels, const uint8_t *__restrict__ gt_difficult,
    const int32_t *__restrict__ n_gt_dev, int G, const int32_t *__restrict__ frame, const double *__restrict__ thr_dev, int T, int C,
    u64 *__restrict__ npos, float *__restrict__ rec_score, int32_t *__restrict__ rec_label, int32_t *__restrict__ rec_image,
    int32_t *__restrict__ rec_pos, uint32_t *__restrict__ rec_flags, long long rec_cap, u64 *__restrict__ cursor, int32_t *__restrict__ err,
    int32_t *__restrict__ ticket, u64 *__restrict__ win, int32_t *__restrict__ ws_match, uint32_t *__restrict__ ws_reach)
{
    __shared__ double s_gx1[EVAL_MAX_G], s_gy1[EVAL_MAX_G], s_gx2[EVAL_MAX_G], s_gy2[EVAL_MAX_G];
    __shared__ int32_t s_glab[EVAL_MAX_G];
    __shared__ double s_thr[EVAL_MAX_T];
    __shared__ int s_last;
    __shared__ u64 s_base;
    const int tid = threadIdx.x;
    const int nc = C - 1;
    const int cnt_raw = *count_dev, ng_raw = *n_gt_dev;
    int e = eval_frame_error(cnt_raw, D, ng_raw, G);                                      // a frame with an error records nothing
    const int n = e ? 0 : cnt_raw;
    const int ng = e ? 0 : (ng_raw < 0 ? 0 : ng_raw);
    const double fw = (double)frame[0], fh = (double)frame[1];
    int bad_label = 0;
    for (int g = tid; g < ng; g += EVAL_THREADS) {
        const float4 b = gt_boxes[g];
        s_gx1[g] = (double)b.x; s_gy1[g] = (double)b.y; s_gx2[g] = (double)b.z; s_gy2[g] = (double)b.w;
        const int l = gt_labels[g];
        s_glab[g] = l;
        if (l < 0 || l >= nc) bad_label = 1;
        else if (blockIdx.x == 0 && !gt_difficult[g]) atomicAdd(&npos[l], 1ull);          // gt_counter_per_class (:46-56)
    }
    if (tid < T) s_thr[tid] = thr_dev[tid];
    __syncthreads();
    // ---- phase 1: the argmax of every detection, and its bid for its match at every threshold it reaches
    for (int i = blockIdx.x * EVAL_THREADS + tid; i < n; i += gridDim.x * EVAL_THREADS) {
        const float4 b = boxes[i];
        const int l = labels[i];
        if (l < 0 || l >= nc) bad_label = 1;
        const double x1 = (double)b.x * fw, y1 = (double)b.y * fh, x2 = (double)b.z * fw, y2 = (double)b.w * fh;      // :90-91
        const double area_d = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
        double ovmax = -1.0;
        int match = -1;
        for (int g = 0; g < ng; ++g) {
            if (s_glab[g] != l) continue;                                                 // :168
            const double gx1 = s_gx1[g], gy1 = s_gy1[g], gx2 = s_gx2[g], gy2 = s_gy2[g];
            const double iw = py_min(x2, gx2) - py_max(x1, gx1) + 1.0;                    // :170-172
            const double ih = py_min(y2, gy2) - py_max(y1, gy1) + 1.0;
            if (iw > 0.0 && ih > 0.0) {
                const double inter = iw * ih;
                const double ua = area_d + (gx2 - gx1 + 1.0) * (gy2 - gy1 + 1.0) - inter; // :175-176
                const double ov = inter / ua;
                if (ov > ovmax) { ovmax = ov; match = g; }                                // :178-180
            }
        }
        uint32_t reach = 0;
        if (match >= 0)
            for (int t = 0; t < T; ++t)
                if (ovmax >= s_thr[t]) reach |= 1u << t;                                  // :184
        ws_match[i] = match;
        ws_reach[i] = reach;
        if (reach && !gt_difficult[match]) {
            const u64 bid = ((u64)eval_orderable(scores[i]) << 32) | (uint32_t)~(uint32_t)i;
            for (int t = 0; t < T; ++t)
                if (reach >> t & 1u) atomicMax(&win[(size_t)t * G + match], bid);
        }
    }
    if (bad_label) e |= EVAL_ERR_LABEL_RANGE;
    if (e) atomicOr(err, e);
    // ---- hand-off to the workgroup that finishes last
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid == 0) {
        agent_st(ticket, 0);        // ready for the next call
        s_base = n > 0 ? atomicAdd(cursor, (u64)n) : 0ull;                                // a full store keeps counting: summarize() reports the loss
    }
    __syncthreads();
    // ---- phase 2: the decision (:184-197) and the records
    const u64 base = s_base;
    const int image_id = frame[2];
    for (int i = tid; i < n; i += EVAL_THREADS) {
        const int match = agent_ld(&ws_match[i]);
        const uint32_t reach = agent_ld(&ws_reach[i]);
        const float sc = scores[i];
        const u64 bid = ((u64)eval_orderable(sc) << 32) | (uint32_t)~(uint32_t)i;
        const bool difficult = match >= 0 && gt_difficult[match];
        uint32_t flags = 0;
        for (int t = 0; t < T; ++t) {
            uint32_t f = FRCNN_EVAL_FP;                                                   // below the threshold, or no same-class ground truth
            if (reach >> t & 1u) {
                if (difficult) f = FRCNN_EVAL_IGNORED;
                else if (agent_ld(&win[(size_t)t * G + match]) == bid) f = FRCNN_EVAL_TP;
            }
            flags |= f << (2 * t);
        }
        const u64 slot = base + (u64)i;
        if (slot < (u64)rec_cap) {
            rec_score[slot] = sc;
            rec_label[slot] = labels[i];
            rec_image[slot] = image_id;
            rec_pos[slot] = i;
            rec_flags[slot] = flags;
        }
    }
    __syncthreads();                                                                      // every winner word has been read
    for (int k = tid; k < T * ng; k += EVAL_THREADS) win[(size_t)(k / ng) * G + (k % ng)] = 0ull;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// average precision (:199-219, voc_ap :115-135)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_THREADS) void eval_ap_kernel(const int32_t *__restrict__ labels, const uint32_t *__restrict__ flags,
                                                               const u64 *__restrict__ n_dev, long long cap, const u64 *__restrict__ npos, int T,
                                                               double *__restrict__ ap, long long *__restrict__ tp_total,
                                                               long long *__restrict__ fp_total, double *__restrict__ prec_ws)
{
    __shared__ u64 s_wave[EVAL_THREADS / 64];
    __shared__ u64 s_carry;
    const int cls = blockIdx.x, nc = (int)gridDim.x;
    const int tid = threadIdx.x;
    const u64 n_raw = *n_dev;
    const long long n = n_raw < (u64)cap ? (long long)n_raw : cap;
    const long long lo = eval_lower_bound(labels, n, cls), hi = eval_lower_bound(labels, n, cls + 1);
    const u64 np = npos[cls];
    double *pk = prec_ws + lo;                                    // the class's own segment: at most hi - lo true positives
    for (int t = 0; t < T; ++t) {
        if (tid == 0) s_carry = 0ull;
        __syncthreads();
        for (long long c0 = lo; c0 < hi; c0 += EVAL_THREADS) {
            const long long i = c0 + tid;
            const uint32_t f = i < hi ? (flags[i] >> (2 * t)) & 3u : 0u;
            const u64 v = eval_scan_step(f, s_wave, &s_carry);    // the cumulative (tp, fp) up to this record
            if (f == FRCNN_EVAL_TP) {
                const long long k = (long long)(v & 0xffffffffull), fpc = (long long)(v >> 32);
                const double den = (double)(k + fpc);             // >= 1 here; the reference's max(., eps) (:217) never binds at a true positive
                pk[k - 1] = (double)k / den;
            }
            eval_scan_carry(v, &s_carry);
        }
        const u64 tot = s_carry;
        const long long K = (long long)(tot & 0xffffffffull);
        __threadfence_block();
        __syncthreads();
        if (tid == 0) {
            tp_total[(size_t)t * nc + cls] = K;
            fp_total[(size_t)t * nc + cls] = (long long)(tot >> 32);
            double a = __builtin_nan("");
            if (np > 0) {
                const double dn = (double)np;
                double m = 0.0;                                   // the end sentinel of prec (:121)
                for (long long k = K; k >= 1; --k) {              // mpre: right-to-left running maximum (:124-125)
                    const double p = pk[k - 1];
                    m = p > m ? p : m;
                    pk[k - 1] = m;
                }
                a = 0.0;
                double prev = 0.0;                                // mrec[0] (:117)
                for (long long k = 1; k <= K; ++k) {              // recall changes at the true positives (:128-134)
                    const double r = (double)k / dn;
                    a = a + (r - prev) * pk[k - 1];
                    prev = r;
                }
                if (1.0 != prev) a = a + (1.0 - prev) * 0.0;      // the end sentinels 1 / 0
            }
            ap[(size_t)t * nc + cls] = a;
        }
        __syncthreads();
    }
}

FRCNN_EXPORT int frcnn_eval_update(const float *boxes, const int32_t *labels, const float *scores, const int32_t *count_dev, int64_t det_capacity,
                                   const float *gt_boxes, const int32_t *gt_labels, const uint8_t *gt_difficult, const int32_t *n_gt_dev,
                                   int64_t gt_capacity, const int32_t *frame_dev, const double *thresholds_dev, int T, int C, int64_t *npos,
                                   float *rec_score, int32_t *rec_label, int32_t *rec_image, int32_t *rec_position, uint32_t *rec_flags,
                                   int64_t record_capacity, int64_t *cursor, int32_t *error_word, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    if (C < 2 || C > EVAL_MAX_C || T < 1 || T > EVAL_MAX_T || !eval_supported(det_capacity, gt_capacity) ||
        det_capacity > (int64_t)(C - 1) * EVAL_MAX_P)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED,
                               "eval_update: C = %d, T = %d, detection capacity %lld, ground-truth capacity %lld outside 2 <= C <= %d, 1 <= T <= %d, "
                               "1 <= D <= (C-1) * %d, 1 <= G <= %d", C, T, (long long)det_capacity, (long long)gt_capacity, EVAL_MAX_C, EVAL_MAX_T,
                               EVAL_MAX_P, EVAL_MAX_G);
    FRCNN_REQUIRE(boxes && labels && scores && count_dev && gt_boxes && gt_labels && gt_difficult && n_gt_dev && frame_dev && thresholds_dev &&
                  npos && rec_score && rec_label && rec_image && rec_position && rec_flags && cursor && error_word && workspace,
                  "eval_update: NULL pointer");
    FRCNN_REQUIRE(record_capacity >= 1, "eval_update: record_capacity must be >= 1");
    FRCNN_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt_boxes & 15) == 0, "eval_update: boxes and gt_boxes must be 16-byte aligned");
    const EvalWs w = eval_ws_layout(det_capacity, gt_capacity, workspace);
    FRCNN_REQUIRE_WS("eval_update", workspace_bytes, w.total);
    int64_t nwg = (det_capacity + EVAL_THREADS - 1) / EVAL_THREADS;
    if (nwg > EVAL_MAX_WG) nwg = EVAL_MAX_WG;
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(eval_update_kernel, dim3((unsigned)nwg), dim3(EVAL_THREADS), 0, s, (const float4 *)boxes, labels, scores, count_dev, (int)det_capacity,
                 (const float4 *)gt_boxes, gt_labels, gt_difficult, n_gt_dev, (int)gt_capacity, frame_dev, thresholds_dev, T, C, (u64 *)npos, rec_score,
                 rec_label, rec_image, rec_position, rec_flags, (long long)record_capacity, (u64 *)cursor, error_word, w.ticket, w.win, w.match,
                 w.reach);
    FRCNN_CHECK_LAUNCH("eval_update_kernel");
    return FRCNN_OK;
}

FRCNN_EXPORT int frcnn_eval_average_precision(const int32_t *labels_sorted, const uint32_t *flags_sorted, const int64_t *n_dev, int64_t capacity,
                                              const int64_t *npos, int T, int C, double *ap, int64_t *tp_total, int64_t *fp_total,
                                              void *workspace, size_t workspace_bytes, void *stream)
{
    if (C < 2 || C > EVAL_MAX_C || T < 1 || T > EVAL_MAX_T)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "eval_average_precision: C = %d, T = %d outside 2 <= C <= %d, 1 <= T <= %d", C, T, EVAL_MAX_C,
                               EVAL_MAX_T);
    FRCNN_REQUIRE(labels_sorted && flags_sorted && n_dev && npos && ap && tp_total && fp_total && workspace, "eval_average_precision: NULL pointer");
    FRCNN_REQUIRE(capacity >= 1, "eval_average_precision: capacity must be >= 1");
    WsCarver c = WsCarver::any_base(workspace);
    double *pw = (double *)c.here();                            // one piece, sized to the byte (not rounded up to the carver's 256)
    FRCNN_REQUIRE_WS("eval_average_precision", workspace_bytes, c.bytes() + (size_t)capacity * sizeof(double));
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(eval_ap_kernel, dim3((unsigned)(C - 1)), dim3(EVAL_THREADS), 0, s, labels_sorted, flags_sorted, (const u64 *)n_dev,
                 (long long)capacity, (const u64 *)npos, T, ap, (long long *)tp_total, (long long *)fp_total, pw);
    FRCNN_CHECK_LAUNCH("eval_ap_kernel");
    return FRCNN_OK;
}
