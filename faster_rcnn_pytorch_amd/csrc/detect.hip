// detect.hip -- the post-processing half of FRCNN.predict (models/model.py:368-402, models/new_model.py:420-470) fused into three
// launches with fixed-capacity outputs and a device count: no host sync, so a whole inference call can be captured into a graph.
//
//   softmax over the head's logits, regression * (0.1, 0.1, 0.2, 0.2), every class decoded against its RoI, clamp to [0, 1]
//   (model.py:368-380), then _suppress (model.py:382-402): per class 1 .. C-1 the candidates prob > thr, torchvision nms(0.3) in
//   descending score (ties: ascending RoI index), and the class-major concatenation with labels l - 1.
//
//  detect_decode_kernel : one wave per RoI row.  The row's softmax (det_expf, a fixed reduction order) and the C-1 decoded boxes
//      (the same frcnn_common.h functions as frcnn_box_codec: bit-identical to predict's op chain), stored class-major ([C-1][P])
//      into the workspace so that the next launch reads one class contiguously.  Rows >= *n_rois_dev are decoded too (they may hold
//      garbage) but never read as detections.
//  detect_nms_kernel    : one workgroup per class.  Candidates of the live rows compacted into LDS as 64-bit keys (score desc, row
//      asc), a bitonic sort, then the greedy scan in score order with nms.hip's exact IoU decision (nms_dev.h); the kept rows are
//      written in order with the class's count.  At most 2048 candidates per class (P <= 2048): 58 KB of LDS.
//  detect_emit_kernel   : one workgroup per class: its output offset (the sum of the counts of the classes before it) and the copy of
//      its kept boxes / scores / labels; the last class writes the total (-1 when the proposal stage reported an aborted scan).
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "nms_dev.h"
#include "detect_dev.h"
FRCNN_LAYOUT_STAMP(detect);

#define DET_MAX_P 2048
#define DET_MAX_C 256
#define DET_THREADS 256

typedef det_u64 u64;

static bool det_supported(int64_t P, int64_t C) { return P >= 1 && P <= DET_MAX_P && C >= 2 && C <= DET_MAX_C; }

// workspace: boxes [C-1][P] float4 | scores [C-1][P] f32 | kept rows [C-1][P] i32 | counts [C-1] i32, each 256-byte aligned
struct DetWs { float4 *box; float *score; int32_t *kept; int32_t *cnt; size_t total; };

static DetWs det_ws_layout(int64_t P, int64_t C, void *workspace)
{
    const size_t n = (size_t)(C - 1) * (size_t)P;
    DetWs w;
    WsCarver c = WsCarver::any_base(workspace);
    w.box = c.get<float4>(n);
    w.score = c.get<float>(n);
    w.kept = c.get<int32_t>(n);
    w.cnt = c.get<int32_t>((size_t)(C - 1));
    w.total = c.bytes();
    return w;
}

size_t frcnn_ws_detect(int64_t P, int64_t C) { return det_supported(P, C) ? det_ws_layout(P, C, nullptr).total : 0; }

__global__ __launch_bounds__(DET_THREADS) void detect_decode_kernel(const float *__restrict__ head_cls, const float *__restrict__ head_reg,
                                                                    const float *__restrict__ rois, int P, int C, float4 *__restrict__ ws_box,
                                                                    float *__restrict__ ws_score, float *__restrict__ out_prob)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (DET_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= P) return;                                           // wave-uniform
    // softmax (model.py:369): NaN anywhere in the row makes the whole row NaN, as torch.softmax does
    const float *x = head_cls + (size_t)r * C;
    float v[DET_MAX_C / 64];
    float m = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < DET_MAX_C / 64; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < C ? x[c] : -__builtin_inff();
        m = tmax(m, v[k]);
    }
    for (int o = 32; o > 0; o >>= 1) m = tmax(m, __shfl_xor(m, o));
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < DET_MAX_C / 64; ++k) {
        v[k] = det_expf(v[k] - m);                                // padding lanes: exp(-inf) = 0
        s = s + v[k];
    }
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);   // butterfly: every lane adds the same pairs, so holds the same sum
    // decode (model.py:372-378): t * (0.1, 0.1, 0.2, 0.2), decode against xy_to_cxcy(roi), cxcy_to_xy, clamp to [0, 1]
    const float *ro = rois + (size_t)r * 4;
    const float4 a = xy_to_cxcy4(make_float4(ro[0], ro[1], ro[2], ro[3]));
#pragma unroll
    for (int k = 0; k < DET_MAX_C / 64; ++k) {
        const int c = lane + 64 * k;
        if (c >= C) break;
        const float p = v[k] / s;
        if (out_prob) out_prob[(size_t)r * C + c] = p;
        if (c == 0) continue;                                     // background: no detections
        const float *t = head_reg + ((size_t)r * C + c) * 4;
        const float4 d = make_float4(t[0] * 0.1f, t[1] * 0.1f, t[2] * 0.2f, t[3] * 0.2f);
        const float4 b = cxcy_to_xy4(decode4(d, a));
        const size_t o = (size_t)(c - 1) * P + r;
        ws_box[o] = make_float4(clamp01(b.x), clamp01(b.y), clamp01(b.z), clamp01(b.w));
        ws_score[o] = p;
    }
}

__global__ __launch_bounds__(DET_THREADS) void detect_nms_kernel(const float4 *__restrict__ ws_box, const float *__restrict__ ws_score,
                                                                 const int32_t *__restrict__ n_dev, int P, float thr_val,
                                                                 const float *__restrict__ thr_dev, float nms_thr, int32_t *__restrict__ ws_kept,
                                                                 int32_t *__restrict__ ws_cnt, int32_t *__restrict__ out_class_counts)
{
    __shared__ u64 s_key[DET_MAX_P];
    __shared__ float4 s_box[DET_MAX_P];
    __shared__ float s_area[DET_MAX_P];
    __shared__ unsigned char s_sup[DET_MAX_P];
    __shared__ int s_m;
    const int cls = blockIdx.x;                                   // class cls + 1 of the head
    const int tid = threadIdx.x;
    int n = *n_dev;
    n = n < 0 ? 0 : (n > P ? P : n);
    const float thr = thr_dev ? *thr_dev : thr_val;
    const size_t base = (size_t)cls * P;
    if (tid == 0) s_m = 0;
    __syncthreads();
    // candidates (model.py:391): the slot order is arbitrary, the sort below makes the result deterministic
    for (int r = tid; r < n; r += DET_THREADS) {
        const float sc = ws_score[base + r];
        if (sc > thr) s_key[atomicAdd(&s_m, 1)] = det_key(sc, (uint32_t)r);
    }
    __syncthreads();
    const int m = s_m;
    int M = 1;
    while (M < m) M <<= 1;
    for (int i = m + tid; i < M; i += DET_THREADS) s_key[i] = ~0ull;
    __syncthreads();
    det_bitonic_sort<DET_THREADS>(s_key, M, tid);                 // ascending: (score desc, row asc), detect_dev.h
    for (int p = tid; p < m; p += DET_THREADS) {
        const float4 b = ws_box[base + (uint32_t)s_key[p]];
        s_box[p] = b;
        s_area[p] = (b.z - b.x) * (b.w - b.y);
        s_sup[p] = 0;
    }
    __syncthreads();
    // greedy NMS in score order (model.py:394): a box is removed by a KEPT box with IoU > nms_thr.  s_sup[i] is final when the scan
    // reaches i (only kept boxes write, each followed by a barrier), so every thread takes the same branch.
    for (int i = 0; i < m; ++i) {
        if (s_sup[i]) continue;
        const float4 bi = s_box[i];
        const float ai = s_area[i];
        for (int j = i + 1 + tid; j < m; j += DET_THREADS)
            if (!s_sup[j] && nms_suppress_exact(bi, ai, s_box[j], s_area[j], nms_thr)) s_sup[j] = 1;
        __syncthreads();
    }
    // the kept rows in score order, by one wave
    if (tid < 64) {
        int cnt = 0;
        for (int b0 = 0; b0 < m; b0 += 64) {
            const int p = b0 + tid;
            const bool keep = p < m && !s_sup[p];
            const u64 mask = __ballot(keep);
            if (keep) ws_kept[base + cnt + __popcll(mask & ((1ull << tid) - 1ull))] = (int32_t)(uint32_t)s_key[p];
            cnt += __popcll(mask);
        }
        if (tid == 0) {
            ws_cnt[cls] = cnt;
            if (out_class_counts) out_class_counts[cls] = cnt;
        }
    }
}

__global__ __launch_bounds__(DET_THREADS) void detect_emit_kernel(const float4 *__restrict__ ws_box, const float *__restrict__ ws_score,
                                                                  const int32_t *__restrict__ ws_kept, const int32_t *__restrict__ ws_cnt,
                                                                  const int32_t *__restrict__ n_dev, int P, float4 *__restrict__ out_boxes,
                                                                  int32_t *__restrict__ out_labels, float *__restrict__ out_scores,
                                                                  int32_t *__restrict__ out_count)
{
    __shared__ int s_off;
    const int cls = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < 64) {                                               // class-major concatenation (model.py:396-402): offset = earlier counts
        int a = 0;
        for (int i = tid; i < cls; i += 64) a += ws_cnt[i];
        a = wave_sum_xor(a);
        if (tid == 0) s_off = a;
    }
    __syncthreads();
    const int off = s_off, cnt = ws_cnt[cls];
    const size_t base = (size_t)cls * P;
    for (int k = tid; k < cnt; k += DET_THREADS) {
        const int r = ws_kept[base + k];
        out_boxes[off + k] = ws_box[base + r];
        out_scores[off + k] = ws_score[base + r];
        out_labels[off + k] = cls;                                // l - 1 (model.py:396)
    }
    if (cls == (int)gridDim.x - 1 && tid == 0) *out_count = *n_dev < 0 ? -1 : off + cnt;
}

FRCNN_EXPORT int frcnn_detect_postprocess(const float *head_cls, const float *head_reg, const float *rois, const int32_t *n_rois_dev,
                                          int64_t P, int C, float threshold, const float *threshold_dev, float nms_threshold,
                                          float *out_boxes, int32_t *out_labels, float *out_scores, int32_t *out_count,
                                          int32_t *out_class_counts, float *out_prob, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!det_supported(P, C))
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "detect_postprocess: P = %lld, C = %d outside 1 <= P <= %d, 2 <= C <= %d", (long long)P, C,
                               DET_MAX_P, DET_MAX_C);
    FRCNN_REQUIRE(head_cls && head_reg && rois && n_rois_dev && out_boxes && out_labels && out_scores && out_count && workspace,
                  "detect_postprocess: NULL pointer");
    FRCNN_REQUIRE(((uintptr_t)out_boxes & 15) == 0, "detect_postprocess: out_boxes must be 16-byte aligned");
    const DetWs w = det_ws_layout(P, C, workspace);
    FRCNN_REQUIRE_WS("detect_postprocess", workspace_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    const int Pi = (int)P;
    FRCNN_LAUNCH(detect_decode_kernel, dim3((unsigned)((P + DET_THREADS / 64 - 1) / (DET_THREADS / 64))), dim3(DET_THREADS), 0, s, head_cls, head_reg,
                 rois, Pi, C, w.box, w.score, out_prob);
    FRCNN_CHECK_LAUNCH("detect_decode_kernel");
    FRCNN_LAUNCH(detect_nms_kernel, dim3((unsigned)(C - 1)), dim3(DET_THREADS), 0, s, (const float4 *)w.box, (const float *)w.score, n_rois_dev, Pi,
                 threshold, threshold_dev, nms_threshold, w.kept, w.cnt, out_class_counts);
    FRCNN_CHECK_LAUNCH("detect_nms_kernel");
    FRCNN_LAUNCH(detect_emit_kernel, dim3((unsigned)(C - 1)), dim3(DET_THREADS), 0, s, (const float4 *)w.box, (const float *)w.score,
                 (const int32_t *)w.kept, (const int32_t *)w.cnt, n_rois_dev, Pi, (float4 *)out_boxes, out_labels, out_scores, out_count);
    FRCNN_CHECK_LAUNCH("detect_emit_kernel");
    return FRCNN_OK;
}
