// detect_merge_dev.h -- what the two class kernels of the merge of detection sets share, so that the greedy scan (detect_merge.hip) and
// the soft-NMS scan (detect_soft.hip) gather, order, fetch, vote and emit with the same instructions: the kernel-argument rows (DmArgs),
// the workspace layout, the candidates of a class in LDS in (score desc, set asc, row asc) order with their flips undone, and the
// copy or box vote of the kept list.  The host half (argument checks, the packing of DmArgs, the emit launch) is defined once in
// detect_merge.hip.
#pragma once
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_host.h"
#include "nms_dev.h"
#include "detect_dev.h"

#define DM_MAX_K FRCNN_MERGE_MAX_SETS
#define DM_MAX_CAND FRCNN_MERGE_MAX_CANDIDATES
#define DM_MAX_C 256
#define DM_THREADS 256
#define DM_ROW_BITS 28                                            // low word of a key: (set << 28) | row
static_assert(DM_MAX_K <= (1 << (32 - DM_ROW_BITS)), "the set index must fit above the row");
static_assert(DM_MAX_CAND <= 65536, "kept positions are stored as 16-bit words");

struct DmArgs {
    const float4 *boxes[DM_MAX_K];
    const int32_t *labels[DM_MAX_K];
    const float *scores[DM_MAX_K];
    const int32_t *counts[DM_MAX_K];
    int32_t caps[DM_MAX_K];
    uint32_t flags[DM_MAX_K];
    int32_t K, pad;
};
static_assert(sizeof(DmArgs) <= 512, "DmArgs and the other arguments must fit well inside the 4 KB kernel-argument segment");

static inline bool dm_supported(int64_t out_capacity, int64_t C) { return out_capacity >= 0 && C >= 2 && C <= DM_MAX_C; }
static inline int64_t dm_stride(int64_t out_capacity) { return out_capacity < 1 ? 1 : (out_capacity < DM_MAX_CAND ? out_capacity : DM_MAX_CAND); }

// workspace: kept boxes [C-1][stride] float4 | kept scores [C-1][stride] f32 | counts [C-1] i32 | status [C-1] u32, each 256-byte aligned
struct DmWs { float4 *box; float *score; int32_t *cnt; uint32_t *status; };

// returns the bytes (sizeof(DmWs) is part of the layout stamp: the struct holds no total)
static inline size_t dm_ws_layout(int64_t out_capacity, int64_t C, void *workspace, DmWs *w)
{
    const size_t n = (size_t)(C - 1) * (size_t)dm_stride(out_capacity);
    WsCarver c = WsCarver::any_base(workspace);
    w->box = c.get<float4>(n);
    w->score = c.get<float>(n);
    w->cnt = c.get<int32_t>((size_t)(C - 1));
    w->status = c.get<uint32_t>((size_t)(C - 1));
    return c.bytes();
}

// detect_merge.hip: frcnn_detect_merge's argument checks under the caller's name `op` (FRCNN_OK, or the error already set), the rows packed
// into *a, the workspace carved into *w, *stride = the workspace's rows per class; and the launch of detect_merge_emit_kernel
int dm_prepare(const char *op, int K, const float *const *boxes, const int32_t *const *labels, const float *const *scores,
               const int32_t *const *counts, const int64_t *caps, const uint32_t *flags, int C, const float *out_boxes, const int32_t *out_labels,
               const float *out_scores, const int32_t *out_count, int64_t out_capacity, void *workspace, size_t workspace_bytes, DmArgs *a, DmWs *w,
               int *stride);
int dm_launch_emit(const DmWs &w, int stride, int64_t out_capacity, int C, float *out_boxes, int32_t *out_labels, float *out_scores,
                   int32_t *out_count, int32_t *out_class_counts, int32_t *out_status, hipStream_t s);

#ifdef __HIPCC__
__device__ __forceinline__ float dm_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

// The candidates of class `cls`: the live rows of every set with that label and score > min_score, compacted into s_key, sorted, their
// boxes (flips undone) and scores fetched into s_box / s_score in sorted order; s_sup (when given) is cleared.  Returns m, the number of
// candidates, 0 with *overflow set when the class held more than DM_MAX_CAND.  *s_status holds the status bits every workgroup finds
// alike.  By the whole workgroup of DM_THREADS threads; ends with a barrier.
__device__ __forceinline__ int dm_gather_sort_fetch(const DmArgs &a, int C, int cls, float min_score, int tid, det_u64 *s_key, float4 *s_box,
                                                    float *s_score, unsigned char *s_sup, int *s_m, unsigned *s_status, bool *overflow)
{
    if (tid == 0) { *s_m = 0; *s_status = 0; }
    __syncthreads();
    // candidates: the slot order is arbitrary, the sort below makes the result deterministic.  Every workgroup walks every live row, so
    // every workgroup finds the same count and label bits.
    unsigned st = 0;
    const int K = a.K < DM_MAX_K ? a.K : DM_MAX_K;
    for (int k = 0; k < K; ++k) {
        int n = *a.counts[k];
        if (n < 0) { st |= FRCNN_MERGE_UPSTREAM_ABORT; n = 0; }
        else if (n > a.caps[k]) { st |= FRCNN_MERGE_COUNT_CLIPPED; n = a.caps[k]; }
        const int32_t *lab = a.labels[k];
        const float *sco = a.scores[k];
        for (int r = tid; r < n; r += DM_THREADS) {
            const int l = lab[r];
            if ((unsigned)l >= (unsigned)(C - 1)) { st |= FRCNN_MERGE_LABEL_RANGE; continue; }
            if (l != cls) continue;
            const float sc = sco[r];
            if (sc > min_score) {
                const int slot = atomicAdd(s_m, 1);
                if (slot < DM_MAX_CAND) s_key[slot] = det_key(sc, ((uint32_t)k << DM_ROW_BITS) | (uint32_t)r);
            }
        }
    }
    if (st) atomicOr(s_status, st);
    __syncthreads();
    int m = *s_m;
    *overflow = m > DM_MAX_CAND;
    if (*overflow) m = 0;                                         // the class comes out empty
    int M = 1;
    while (M < m) M <<= 1;
    for (int i = m + tid; i < M; i += DM_THREADS) s_key[i] = ~0ull;
    __syncthreads();
    det_bitonic_sort<DM_THREADS>(s_key, M, tid);                  // ascending: (score desc, set asc, row asc)
    for (int p = tid; p < m; p += DM_THREADS) {
        const uint32_t low = (uint32_t)s_key[p];
        const int k = (int)(low >> DM_ROW_BITS), r = (int)(low & ((1u << DM_ROW_BITS) - 1u));
        float4 b = a.boxes[k][r];
        const uint32_t f = a.flags[k];
        if (f & 1u) { const float x1 = 1.0f - b.z, x2 = 1.0f - b.x; b.x = x1; b.z = x2; }
        if (f & 2u) { const float y1 = 1.0f - b.w, y2 = 1.0f - b.y; b.y = y1; b.w = y2; }
        s_box[p] = b;
        s_score[p] = a.scores[k][r];
        if (s_sup) s_sup[p] = 0;
    }
    __syncthreads();
    return m;
}

// One wave per kept box: the box itself, or the score-weighted mean of its voters in the order include/frcnn_hip.h states, to row q of the
// class's workspace.  The voters' weights are the candidates' own scores (s_score); the score written is s_kscore[q] when given (the
// working score of a soft scan), else the kept candidate's own.
__device__ __forceinline__ void dm_vote_copy(int cls, int tid, int m, int nkept, float vote_thr, int stride, const float4 *s_box,
                                             const float *s_score, const unsigned short *s_kept, const float *s_kscore,
                                             float4 *__restrict__ ws_box, float *__restrict__ ws_score)
{
    const int lane = tid & 63;
    const bool voting = vote_thr >= 0.0f;                         // false for NaN
    for (int q = tid >> 6; q < nkept; q += DM_THREADS / 64) {     // wave-uniform
        const int pi = s_kept[q];
        const float4 bi = s_box[pi];
        float4 res = bi;
        if (voting) {
            const float ai = dm_area(bi);
            double sw = 0.0, sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
            int voters = 0;
            for (int p = lane; p < m; p += 64) {
                const float4 bj = s_box[p];
                if (p == pi || nms_iou_exact(bi, ai, bj, dm_area(bj)) >= vote_thr) {
                    const double s = (double)s_score[p];
                    sw = __dadd_rn(sw, s);
                    sx1 = __dadd_rn(sx1, __dmul_rn(s, (double)bj.x));
                    sy1 = __dadd_rn(sy1, __dmul_rn(s, (double)bj.y));
                    sx2 = __dadd_rn(sx2, __dmul_rn(s, (double)bj.z));
                    sy2 = __dadd_rn(sy2, __dmul_rn(s, (double)bj.w));
                    ++voters;
                }
            }
            sw = wave_sum_xor(sw);
            sx1 = wave_sum_xor(sx1);
            sy1 = wave_sum_xor(sy1);
            sx2 = wave_sum_xor(sx2);
            sy2 = wave_sum_xor(sy2);
            voters = wave_sum_xor(voters);
            const bool finite = isfinite(sw) && isfinite(sx1) && isfinite(sy1) && isfinite(sx2) && isfinite(sy2);
            if (voters > 1 && finite && sw > 0.0)
                res = make_float4((float)__ddiv_rn(sx1, sw), (float)__ddiv_rn(sy1, sw), (float)__ddiv_rn(sx2, sw), (float)__ddiv_rn(sy2, sw));
        }
        if (lane == 0 && q < stride) {
            const size_t o = (size_t)cls * stride + q;
            ws_box[o] = res;
            ws_score[o] = s_kscore ? s_kscore[q] : s_score[pi];
        }
    }
}
#endif  // __HIPCC__
