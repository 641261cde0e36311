// detect_soft.hip -- Soft-NMS (Bodla et al., 2017) as the suppression step of the merge of detection sets: frcnn_detect_merge_soft is
// frcnn_detect_merge with the greedy scan replaced by a scan that DECAYS the scores of the boxes a picked box overlaps.  The contract is
// this project's and is stated in include/frcnn_hip.h.  Everything but the scan is detect_merge.hip's, by the same instructions
// (detect_merge_dev.h): the gather, the order, the box fetch, the copy or vote of the kept list, the workspace, the emit kernel.  Two
// launches whatever the data holds, no host sync, capturable.
//
//  detect_soft_class_kernel<METHOD> : one workgroup of 256 threads per class.  After the shared gather / sort / fetch, thread t owns the
//      sorted positions t, t + 256, ... (at most 8): box, area and working score in registers (48 VGPRs; the slot loops are fully unrolled
//      under the uniform bound ceil(m / 256), so the arrays never leave the register file) and a live mask.  The sorted boxes stay in LDS
//      as well: the picked box is one broadcast read.  A decay can reorder the remaining candidates, so one sort up front is not enough:
//      every step is a block-wide arg-max over the decayed scores.  Per step: each thread forms the best key over its live slots -- the
//      complement of det_key(working score, position), so that the larger word is the better candidate and 0 means "none" --
//      wave_max_dpp reduces it (frcnn_dev.h's DPP chain on both halves of the word: 6-10 % off the step against the xor butterfly,
//      measured), lane 63 of each wave stores it in a parity-double-buffered LDS row, ONE barrier, every thread reads the four words and
//      takes the best; the owner retires the winner and appends (position, working score) to the kept list; every thread decays
//      its own live slots against the winner.  The loop ends when no wave reports a live key.  Why one barrier is enough: step n writes
//      row n & 1 and reads it after barrier n; row n & 1 is written again in step n + 2, which a wave reaches only through barrier n + 1,
//      that is after every wave has read row n & 1.
//
// Cost: one step per emitted candidate (the greedy scan skips suppressed boxes, this one cannot skip a decayed one), each ceil(m / 256)
// IoUs per thread, a 6-step 64-bit DPP chain and a barrier.  LDS: 60 KB (keys 16 -- reused for the kept scores once the boxes are fetched -- boxes 32, scores 8,
// kept positions 4) + 64 bytes of reduction rows.  No atomics on global memory, no workgroup waits on another.  The library is built with
// -ffp-contract=off: a decay is the fp32 operations the header names, each rounded.
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "nms_dev.h"
#include "detect_dev.h"
#include "detect_merge_dev.h"
FRCNN_LAYOUT_STAMP(detect_soft);

#define DS_SLOTS (DM_MAX_CAND / DM_THREADS)
#define DS_WAVES (DM_THREADS / 64)
static_assert(DS_SLOTS * DM_THREADS == DM_MAX_CAND && DS_SLOTS <= 32, "the live mask is one 32-bit word");
static_assert(sizeof(det_u64) * DM_MAX_CAND >= sizeof(float) * DM_MAX_CAND, "the kept scores reuse the keys' LDS");

template <int METHOD>
__global__ __launch_bounds__(DM_THREADS) void detect_soft_class_kernel(const DmArgs a, int C, float min_score, float nms_thr, float sigma,
                                                                      float score_floor, float vote_thr, int stride, float4 *__restrict__ ws_box,
                                                                      float *__restrict__ ws_score, int32_t *__restrict__ ws_cnt,
                                                                      uint32_t *__restrict__ ws_status)
{
    __shared__ det_u64 s_key[DM_MAX_CAND];
    __shared__ float4 s_box[DM_MAX_CAND];
    __shared__ float s_score[DM_MAX_CAND];
    __shared__ unsigned short s_kept[DM_MAX_CAND];
    __shared__ det_u64 s_red[2][DS_WAVES];
    __shared__ int s_m;
    __shared__ unsigned s_status;
    const int cls = blockIdx.x;
    const int tid = threadIdx.x;
    bool overflow;
    const int m = dm_gather_sort_fetch(a, C, cls, min_score, tid, s_key, s_box, s_score, nullptr, &s_m, &s_status, &overflow);
    float *s_kscore = (float *)s_key;                             // the keys were last read before the fetch's closing barrier
    const int nslots = (m + DM_THREADS - 1) / DM_THREADS;         // uniform
    float4 box[DS_SLOTS];
    float area[DS_SLOTS], w[DS_SLOTS];
    unsigned live = 0;
#pragma unroll
    for (int s = 0; s < DS_SLOTS; ++s) {
        box[s] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        area[s] = 0.0f;
        w[s] = 0.0f;
        if (s < nslots) {
            const int p = tid + s * DM_THREADS;
            if (p < m) {
                box[s] = s_box[p];
                area[s] = dm_area(box[s]);
                w[s] = s_score[p];
                live |= 1u << s;
            }
        }
    }
    int n = 0;                                                    // emitted so far: uniform
    for (;;) {
        det_u64 best = 0;
#pragma unroll
        for (int s = 0; s < DS_SLOTS; ++s)
            if (s < nslots && ((live >> s) & 1u)) {
                const det_u64 k = ~det_key(w[s], (uint32_t)(tid + s * DM_THREADS));
                best = k > best ? k : best;
            }
        best = wave_max_dpp(best);                                // lane 63 holds the wave's best
        if ((tid & 63) == 63) s_red[n & 1][tid >> 6] = best;
        __syncthreads();
        best = 0;
#pragma unroll
        for (int v = 0; v < DS_WAVES; ++v) {
            const det_u64 k = s_red[n & 1][v];
            best = k > best ? k : best;
        }
        if (best == 0) break;                                     // no live candidate anywhere: every thread leaves together
        const int p = (int)(uint32_t)~best;                       // the key's low word: the winner's sorted position, < m
        const float4 bp = s_box[p];
        const float ap = dm_area(bp);
        const bool own = (p & (DM_THREADS - 1)) == tid;
        const int ps = p / DM_THREADS;
#pragma unroll
        for (int s = 0; s < DS_SLOTS; ++s)
            if (s < nslots) {
                const unsigned bit = 1u << s;
                if (own && s == ps) {                             // retire the winner: position and working score to the kept list
                    live &= ~bit;
                    s_kept[n] = (unsigned short)p;
                    s_kscore[n] = w[s];
                } else if (live & bit) {
                    const float ov = nms_iou_exact(bp, ap, box[s], area[s]);
                    if (METHOD == FRCNN_SOFT_NMS_HARD) {
                        if (ov > nms_thr) live &= ~bit;
                    } else if (METHOD == FRCNN_SOFT_NMS_LINEAR) {
                        if (ov > nms_thr) {
                            const float keep = 1.0f - ov;
                            w[s] = w[s] * keep;
                            if (!(w[s] >= score_floor)) live &= ~bit;
                        }
                    } else {
                        if (ov > 0.0f) {
                            const double q = __ddiv_rn(__dmul_rn((double)ov, (double)ov), (double)sigma);
                            const float keep = (float)exp(-q);
                            w[s] = w[s] * keep;
                            if (!(w[s] >= score_floor)) live &= ~bit;
                        }
                    }
                }
            }
        ++n;
    }
    // the kept list is complete and visible: its last entry was written before the barrier of the step that found nothing live
    if (tid == 0) {
        ws_cnt[cls] = n;
        ws_status[cls] = s_status | (overflow ? FRCNN_MERGE_CLASS_OVERFLOW : 0u);
    }
    dm_vote_copy(cls, tid, m, n, vote_thr, stride, s_box, s_score, s_kept, s_kscore, ws_box, ws_score);
}

FRCNN_EXPORT int frcnn_detect_merge_soft(int K, const float *const *boxes, const int32_t *const *labels, const float *const *scores,
                                         const int32_t *const *counts, const int64_t *caps, const uint32_t *flags, int C, float min_score,
                                         float nms_threshold, float vote_threshold, int method, float sigma, float score_floor, float *out_boxes,
                                         int32_t *out_labels, float *out_scores, int32_t *out_count, int32_t *out_class_counts, int32_t *out_status,
                                         int64_t out_capacity, void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(method >= FRCNN_SOFT_NMS_HARD && method <= FRCNN_SOFT_NMS_GAUSSIAN, "detect_merge_soft: method = %d outside 0 .. 2", method);
    FRCNN_REQUIRE(method != FRCNN_SOFT_NMS_GAUSSIAN || sigma > 0.0f, "detect_merge_soft: sigma = %g must be > 0 in gaussian mode", (double)sigma);
    FRCNN_REQUIRE(score_floor == score_floor, "detect_merge_soft: score_floor is NaN");
    DmArgs a;
    DmWs w;
    int stride;
    const int rc = dm_prepare("detect_merge_soft", K, boxes, labels, scores, counts, caps, flags, C, out_boxes, out_labels, out_scores, out_count,
                              out_capacity, workspace, workspace_bytes, &a, &w, &stride);
    if (rc != FRCNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(C - 1)), block(DM_THREADS);
    if (method == FRCNN_SOFT_NMS_HARD)
        FRCNN_LAUNCH(detect_soft_class_kernel<FRCNN_SOFT_NMS_HARD>, grid, block, 0, s, a, C, min_score, nms_threshold, sigma, score_floor,
                     vote_threshold, stride, w.box, w.score, w.cnt, w.status);
    else if (method == FRCNN_SOFT_NMS_LINEAR)
        FRCNN_LAUNCH(detect_soft_class_kernel<FRCNN_SOFT_NMS_LINEAR>, grid, block, 0, s, a, C, min_score, nms_threshold, sigma, score_floor,
                     vote_threshold, stride, w.box, w.score, w.cnt, w.status);
    else
        FRCNN_LAUNCH(detect_soft_class_kernel<FRCNN_SOFT_NMS_GAUSSIAN>, grid, block, 0, s, a, C, min_score, nms_threshold, sigma, score_floor,
                     vote_threshold, stride, w.box, w.score, w.cnt, w.status);
    FRCNN_CHECK_LAUNCH("detect_soft_class_kernel");
    return dm_launch_emit(w, stride, out_capacity, C, out_boxes, out_labels, out_scores, out_count, out_class_counts, out_status, s);
}
