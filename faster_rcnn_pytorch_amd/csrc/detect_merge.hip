// detect_merge.hip -- K fixed-capacity detection sets with device counts merged into one set of the same shape: the merge step of
// test-time augmentation (a mirrored view, further scales), of ensembling two weight sets, and of anything else that sees one frame
// more than once.  The reference has no such step (its test loop sees one view, test.py:60); the contract is this project's and is
// stated in include/frcnn_hip.h.  Two launches whatever the data holds, no host sync, capturable.
//
//  detect_merge_class_kernel : one workgroup per class.  The live rows of every set with that label and score > min_score are compacted
//      into LDS as 64-bit keys (score desc, set asc, row asc: detect_dev.h's key with (set << 28) | row as its low word), sorted by
//      detect.hip's bitonic sort, their boxes fetched with the view's flip undone, then detect_nms_kernel's greedy scan with nms_dev.h's
//      exact decision.  One wave per kept box then either copies it or replaces it by the score-weighted mean of its voters (box voting):
//      binary64 sums in the fixed order the header states.  The kept rows go to the workspace, [C-1][stride] with
//      stride = min(2048, out_capacity).
//  detect_merge_emit_kernel  : one workgroup per class: its output offset (the sum of the counts of the classes before it) and the copy of
//      its rows, bounded by out_capacity; the last class writes the total and the status word.
//
// The K rows of pointers, capacities and flags travel BY VALUE in the kernel arguments (DmArgs, 272 bytes), as grad_accum.hip's rows do: a
// graph node stores them, so nothing host-side is read at replay time.  The set index is uniform, so the rows are read with scalar loads.
//
// Memory: every class workgroup reads the labels of all live rows (4 B each, from L2 after the first workgroup) and the score and box of
// its own candidates once; the scan and the voting run out of LDS: 62 KB (keys 16, boxes 32, scores 8, kept positions 4, flags 2).  No
// atomics on global memory, no workgroup waits on another.  The library is built with -ffp-contract=off; the binary64 adds are written
// out (__dadd_rn).
//
// What the class kernel shares with the soft-NMS scan of detect_soft.hip -- DmArgs, the workspace layout, the gather / sort / fetch, the
// copy or vote of the kept list -- lives in detect_merge_dev.h; the argument checks (dm_prepare) and the emit launch (dm_launch_emit) are
// defined here and serve both entry points.
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "nms_dev.h"
#include "detect_dev.h"
#include "detect_merge_dev.h"
FRCNN_LAYOUT_STAMP(detect_merge);

size_t frcnn_ws_detect_merge(int64_t out_capacity, int64_t C)
{
    DmWs w;
    return dm_supported(out_capacity, C) ? dm_ws_layout(out_capacity, C, nullptr, &w) : 0;
}

__global__ __launch_bounds__(DM_THREADS) void detect_merge_class_kernel(const DmArgs a, int C, float min_score, float nms_thr, float vote_thr,
                                                                       int stride, float4 *__restrict__ ws_box, float *__restrict__ ws_score,
                                                                       int32_t *__restrict__ ws_cnt, uint32_t *__restrict__ ws_status)
{
    __shared__ det_u64 s_key[DM_MAX_CAND];
    __shared__ float4 s_box[DM_MAX_CAND];
    __shared__ float s_score[DM_MAX_CAND];
    __shared__ unsigned short s_kept[DM_MAX_CAND];
    __shared__ unsigned char s_sup[DM_MAX_CAND];
    __shared__ int s_m, s_nkept;
    __shared__ unsigned s_status;
    const int cls = blockIdx.x;
    const int tid = threadIdx.x;
    bool overflow;
    const int m = dm_gather_sort_fetch(a, C, cls, min_score, tid, s_key, s_box, s_score, s_sup, &s_m, &s_status, &overflow);
    // greedy NMS in that order, as detect_nms_kernel: s_sup[i] is final when the scan reaches i (only kept boxes write, each followed by a
    // barrier), so every thread takes the same branch
    for (int i = 0; i < m; ++i) {
        if (s_sup[i]) continue;
        const float4 bi = s_box[i];
        const float ai = dm_area(bi);
        for (int j = i + 1 + tid; j < m; j += DM_THREADS)
            if (!s_sup[j]) {
                const float4 bj = s_box[j];
                if (nms_suppress_exact(bi, ai, bj, dm_area(bj), nms_thr)) s_sup[j] = 1;
            }
        __syncthreads();
    }
    // the kept positions in order, by one wave
    if (tid < 64) {
        int cnt = 0;
        for (int b0 = 0; b0 < m; b0 += 64) {
            const int p = b0 + tid;
            const bool keep = p < m && !s_sup[p];
            const det_u64 mask = __ballot(keep);
            if (keep) s_kept[cnt + __popcll(mask & ((1ull << tid) - 1ull))] = (unsigned short)p;
            cnt += __popcll(mask);
        }
        if (tid == 0) {
            s_nkept = cnt;
            ws_cnt[cls] = cnt;
            ws_status[cls] = s_status | (overflow ? FRCNN_MERGE_CLASS_OVERFLOW : 0u);
        }
    }
    __syncthreads();
    // one wave per kept box: the box itself, or the score-weighted mean of its voters in the order include/frcnn_hip.h states
    dm_vote_copy(cls, tid, m, s_nkept, vote_thr, stride, s_box, s_score, s_kept, nullptr, ws_box, ws_score);
}

__global__ __launch_bounds__(DM_THREADS) void detect_merge_emit_kernel(const float4 *__restrict__ ws_box, const float *__restrict__ ws_score,
                                                                      const int32_t *__restrict__ ws_cnt, const uint32_t *__restrict__ ws_status,
                                                                      int stride, long long out_capacity, float4 *__restrict__ out_boxes,
                                                                      int32_t *__restrict__ out_labels, float *__restrict__ out_scores,
                                                                      int32_t *__restrict__ out_count, int32_t *__restrict__ out_class_counts,
                                                                      int32_t *__restrict__ out_status)
{
    __shared__ int s_off;
    const int cls = blockIdx.x;
    const int tid = threadIdx.x;
    const bool last = cls == (int)gridDim.x - 1;
    if (tid < 64) {                                               // class-major concatenation: offset = the earlier classes' counts
        int a = 0;
        unsigned st = 0;
        for (int i = tid; i < cls; i += 64) a += ws_cnt[i];
        a = wave_sum_xor(a);
        if (last) {                                               // block-uniform
            for (int i = tid; i < (int)gridDim.x; i += 64) st |= ws_status[i];
            st = wave_reduce_xor(st, [](unsigned x, unsigned y) { return x | y; });
        }
        if (tid == 0) {
            s_off = a;
            const int cnt = ws_cnt[cls];
            if (out_class_counts) out_class_counts[cls] = cnt;
            if (last) {
                const int total = a + cnt;                        // <= 255 * 2048
                if ((long long)total > out_capacity) st |= FRCNN_MERGE_OUTPUT_OVERFLOW;
                const unsigned fatal = FRCNN_MERGE_UPSTREAM_ABORT | FRCNN_MERGE_CLASS_OVERFLOW | FRCNN_MERGE_OUTPUT_OVERFLOW;
                *out_count = (st & fatal) ? -1 : total;
                if (out_status) *out_status = (int32_t)st;
            }
        }
    }
    __syncthreads();
    const int off = s_off, cnt = ws_cnt[cls];
    const size_t base = (size_t)cls * stride;
    for (int k = tid; k < cnt; k += DM_THREADS) {
        if (k >= stride || (long long)off + k >= out_capacity) break;     // rows past out_capacity: never written (stride <= out_capacity)
        out_boxes[off + k] = ws_box[base + k];
        out_scores[off + k] = ws_score[base + k];
        out_labels[off + k] = cls;
    }
}

int dm_prepare(const char *op, int K, const float *const *boxes, const int32_t *const *labels, const float *const *scores,
               const int32_t *const *counts, const int64_t *caps, const uint32_t *flags, int C, const float *out_boxes, const int32_t *out_labels,
               const float *out_scores, const int32_t *out_count, int64_t out_capacity, void *workspace, size_t workspace_bytes, DmArgs *a, DmWs *w,
               int *stride)
{
    FRCNN_REQUIRE(K >= 1 && K <= DM_MAX_K, "%s: K = %d outside 1 .. %d", op, K, DM_MAX_K);
    FRCNN_REQUIRE(boxes && labels && scores && counts && caps && flags && out_boxes && out_labels && out_scores && out_count && workspace,
                  "%s: NULL pointer", op);
    FRCNN_REQUIRE(out_capacity >= 0, "%s: negative out_capacity", op);
    FRCNN_REQUIRE(((uintptr_t)out_boxes & 15) == 0, "%s: out_boxes must be 16-byte aligned", op);
    for (int k = 0; k < K; ++k) {
        FRCNN_REQUIRE(boxes[k] && labels[k] && scores[k] && counts[k], "%s: NULL pointer in set %d", op, k);
        FRCNN_REQUIRE(caps[k] >= 0, "%s: negative capacity of set %d", op, k);
        FRCNN_REQUIRE(((uintptr_t)boxes[k] & 15) == 0, "%s: the boxes of set %d must be 16-byte aligned", op, k);
    }
    if (C < 2 || C > DM_MAX_C) return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "%s: C = %d outside 2 .. %d", op, C, DM_MAX_C);
    for (int k = 0; k < K; ++k)
        if (caps[k] > ((int64_t)1 << DM_ROW_BITS))
            return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "%s: capacity %lld of set %d above 2^%d", op, (long long)caps[k], k, DM_ROW_BITS);
    FRCNN_REQUIRE_WS(op, workspace_bytes, dm_ws_layout(out_capacity, C, workspace, w));
    *a = DmArgs{};
    for (int k = 0; k < K; ++k) {
        a->boxes[k] = (const float4 *)boxes[k];
        a->labels[k] = labels[k];
        a->scores[k] = scores[k];
        a->counts[k] = counts[k];
        a->caps[k] = (int32_t)caps[k];
        a->flags[k] = flags[k];
    }
    a->K = K;
    *stride = (int)dm_stride(out_capacity);
    return FRCNN_OK;
}

int dm_launch_emit(const DmWs &w, int stride, int64_t out_capacity, int C, float *out_boxes, int32_t *out_labels, float *out_scores,
                   int32_t *out_count, int32_t *out_class_counts, int32_t *out_status, hipStream_t s)
{
    FRCNN_LAUNCH(detect_merge_emit_kernel, dim3((unsigned)(C - 1)), dim3(DM_THREADS), 0, s, (const float4 *)w.box, (const float *)w.score,
                 (const int32_t *)w.cnt, (const uint32_t *)w.status, stride, (long long)out_capacity, (float4 *)out_boxes, out_labels, out_scores,
                 out_count, out_class_counts, out_status);
    FRCNN_CHECK_LAUNCH("detect_merge_emit_kernel");
    return FRCNN_OK;
}

FRCNN_EXPORT int frcnn_detect_merge(int K, const float *const *boxes, const int32_t *const *labels, const float *const *scores,
                                    const int32_t *const *counts, const int64_t *caps, const uint32_t *flags, int C, float min_score,
                                    float nms_threshold, float vote_threshold, float *out_boxes, int32_t *out_labels, float *out_scores,
                                    int32_t *out_count, int32_t *out_class_counts, int32_t *out_status, int64_t out_capacity, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    DmArgs a;
    DmWs w;
    int stride;
    const int rc = dm_prepare("detect_merge", K, boxes, labels, scores, counts, caps, flags, C, out_boxes, out_labels, out_scores, out_count,
                              out_capacity, workspace, workspace_bytes, &a, &w, &stride);
    if (rc != FRCNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(detect_merge_class_kernel, dim3((unsigned)(C - 1)), dim3(DM_THREADS), 0, s, a, C, min_score, nms_threshold, vote_threshold, stride,
                 w.box, w.score, w.cnt, w.status);
    FRCNN_CHECK_LAUNCH("detect_merge_class_kernel");
    return dm_launch_emit(w, stride, out_capacity, C, out_boxes, out_labels, out_scores, out_count, out_class_counts, out_status, s);
}
