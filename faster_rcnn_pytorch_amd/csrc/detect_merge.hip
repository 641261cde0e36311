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
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "nms_dev.h"
#include "detect_dev.h"
FRCNN_LAYOUT_STAMP(detect_merge);

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

static bool dm_supported(int64_t out_capacity, int64_t C) { return out_capacity >= 0 && C >= 2 && C <= DM_MAX_C; }
static int64_t dm_stride(int64_t out_capacity) { return out_capacity < 1 ? 1 : (out_capacity < DM_MAX_CAND ? out_capacity : DM_MAX_CAND); }

// workspace: kept boxes [C-1][stride] float4 | kept scores [C-1][stride] f32 | counts [C-1] i32 | status [C-1] u32, each 256-byte aligned
struct DmWs { float4 *box; float *score; int32_t *cnt; uint32_t *status; };

static size_t dm_ws_layout(int64_t out_capacity, int64_t C, char *base, DmWs *w)
{
    const size_t n = (size_t)(C - 1) * (size_t)dm_stride(out_capacity);
    size_t off = 0;
    if (w) w->box = (float4 *)(base + off);
    off += align_up(n * sizeof(float4), 256);
    if (w) w->score = (float *)(base + off);
    off += align_up(n * sizeof(float), 256);
    if (w) w->cnt = (int32_t *)(base + off);
    off += align_up((size_t)(C - 1) * sizeof(int32_t), 256);
    if (w) w->status = (uint32_t *)(base + off);
    off += align_up((size_t)(C - 1) * sizeof(uint32_t), 256);
    return off;
}

size_t frcnn_ws_detect_merge(int64_t out_capacity, int64_t C)
{
    if (!dm_supported(out_capacity, C)) return 0;
    return 256 + dm_ws_layout(out_capacity, C, nullptr, nullptr);  // + the slack that aligns the caller's pointer
}

__device__ __forceinline__ float dm_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

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
    if (tid == 0) { s_m = 0; s_status = 0; }
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
                const int slot = atomicAdd(&s_m, 1);
                if (slot < DM_MAX_CAND) s_key[slot] = det_key(sc, ((uint32_t)k << DM_ROW_BITS) | (uint32_t)r);
            }
        }
    }
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    int m = s_m;
    const bool overflow = m > DM_MAX_CAND;
    if (overflow) m = 0;                                          // the class comes out empty
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
        s_sup[p] = 0;
    }
    __syncthreads();
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
    const int nkept = s_nkept;
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
            ws_score[o] = s_score[pi];
        }
    }
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

FRCNN_EXPORT int frcnn_detect_merge(int K, const float *const *boxes, const int32_t *const *labels, const float *const *scores,
                                    const int32_t *const *counts, const int64_t *caps, const uint32_t *flags, int C, float min_score,
                                    float nms_threshold, float vote_threshold, float *out_boxes, int32_t *out_labels, float *out_scores,
                                    int32_t *out_count, int32_t *out_class_counts, int32_t *out_status, int64_t out_capacity, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(K >= 1 && K <= DM_MAX_K, "detect_merge: K = %d outside 1 .. %d", K, DM_MAX_K);
    FRCNN_REQUIRE(boxes && labels && scores && counts && caps && flags && out_boxes && out_labels && out_scores && out_count && workspace,
                  "detect_merge: NULL pointer");
    FRCNN_REQUIRE(out_capacity >= 0, "detect_merge: negative out_capacity");
    FRCNN_REQUIRE(((uintptr_t)out_boxes & 15) == 0, "detect_merge: out_boxes must be 16-byte aligned");
    for (int k = 0; k < K; ++k) {
        FRCNN_REQUIRE(boxes[k] && labels[k] && scores[k] && counts[k], "detect_merge: NULL pointer in set %d", k);
        FRCNN_REQUIRE(caps[k] >= 0, "detect_merge: negative capacity of set %d", k);
        FRCNN_REQUIRE(((uintptr_t)boxes[k] & 15) == 0, "detect_merge: the boxes of set %d must be 16-byte aligned", k);
    }
    if (C < 2 || C > DM_MAX_C) return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "detect_merge: C = %d outside 2 .. %d", C, DM_MAX_C);
    for (int k = 0; k < K; ++k)
        if (caps[k] > ((int64_t)1 << DM_ROW_BITS))
            return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "detect_merge: capacity %lld of set %d above 2^%d", (long long)caps[k], k, DM_ROW_BITS);
    const size_t need = frcnn_ws_detect_merge(out_capacity, C);
    if (workspace_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "detect_merge: workspace %zu < %zu bytes", workspace_bytes, need);
    DmWs w;
    char *base = (char *)workspace + (align_up((uintptr_t)workspace, 256) - (uintptr_t)workspace);
    dm_ws_layout(out_capacity, C, base, &w);
    DmArgs a = {};
    for (int k = 0; k < K; ++k) {
        a.boxes[k] = (const float4 *)boxes[k];
        a.labels[k] = labels[k];
        a.scores[k] = scores[k];
        a.counts[k] = counts[k];
        a.caps[k] = (int32_t)caps[k];
        a.flags[k] = flags[k];
    }
    a.K = K;
    hipStream_t s = (hipStream_t)stream;
    const int stride = (int)dm_stride(out_capacity);
    FRCNN_LAUNCH(detect_merge_class_kernel, dim3((unsigned)(C - 1)), dim3(DM_THREADS), 0, s, a, C, min_score, nms_threshold, vote_threshold, stride,
                 w.box, w.score, w.cnt, w.status);
    FRCNN_CHECK_LAUNCH("detect_merge_class_kernel");
    FRCNN_LAUNCH(detect_merge_emit_kernel, dim3((unsigned)(C - 1)), dim3(DM_THREADS), 0, s, (const float4 *)w.box, (const float *)w.score,
                 (const int32_t *)w.cnt, (const uint32_t *)w.status, stride, (long long)out_capacity, (float4 *)out_boxes, out_labels, out_scores,
                 out_count, out_class_counts, out_status);
    FRCNN_CHECK_LAUNCH("detect_merge_emit_kernel");
    return FRCNN_OK;
}
