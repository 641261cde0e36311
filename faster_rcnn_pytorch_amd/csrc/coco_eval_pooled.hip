// coco_eval_pooled.hip -- the COCO bbox protocol with every category pooled (pycocotools' COCOeval with useCats = 0): what proposal recall
// (AR@100 / 300 / 1000) and class-agnostic detection AP are measured with.  One frame, two launches whatever the data holds, no host sync,
// no workgroup that waits on another; the records go to the store of coco_eval.hip and are accumulated by its coco_accumulate_kernel with K = 1.
//
// A frame's detections and its ground truths are each ONE list in the order (label ascending, original position ascending); labels only
// order the lists and are range-checked.  The detections are ranked by score descending, stable over that pooled order, and cut to
// max_det (<= EVAL_MAX_P).  Pixel boxes, the float64 IoU, the area ranges and gtIg are those of coco_update_kernel; a detection may match a
// ground truth of any label.
//
//  coco_pooled_rank_kernel  : one workgroup, once per frame.  Checks the counts and labels (a frame with an error bit is not recorded: the
//      header says nd = 0 and the second launch does nothing); sorts the ground truths' (label, position) keys -- a bitonic network in LDS --
//      into the pooled order gperm[]; adds the non-ignored ground truths to npig[0][a]; packs the detections' keys (orderable(score) << 32 |
//      ~(label << 20 | position): unique, and descending = score descending, label ascending, position ascending), takes the max_det
//      largest (a radix select over the workspace when there are more) and orders them with the same network; forms the ranked detections'
//      float64 pixel xywh boxes; reserves the frame's slots with one atomic add on the cursor and writes the records with rec_label = 0,
//      rec_rank = the pooled rank and all four flag words ZERO.
//  coco_pooled_match_kernel : one workgroup per (area range, threshold) chain.  A thread keeps four ground truths (pooled index tid + 256 i)
//      and their matched bits in registers.  The chain walks the detections in rank order; a step is evaluateImg's walk over the ground
//      truths for one detection, in its two-pass form, as ONE block-wide arg-max: every thread computes the IoUs of its eligible ground
//      truths (not matched, or crowd; IoU >= min(t, 1 - 1e-10)) and the workgroup takes the maximum of the key (not ignored, IoU, pooled
//      index) -- "< best: continue" keeps the LAST maximum, which is the larger pooled index; a non-ignored candidate beats every ignored
//      one, which is the second pass running only when the first matched nothing.  A DPP chain per wave, then four words through LDS: one
//      barrier per detection (the words alternate), so a chain costs nd steps, not nd * G; waves without a live ground truth only keep
//      the barriers.  The chain's 2-bit codes are collected in LDS and ORed into the records' flag words with ordinary vector
//      atomics at the end: the T chains of an area range share a word, which the first launch of the same call has zeroed.
//
// Workspace (frcnn_workspace_bytes(FRCNN_OP_COCO_EVAL_POOLED, D, G)): header, gperm, the ranked detections' boxes and the packed keys.  ANY
// content between calls: every word the second launch reads is written by the first launch of the same call.
#include "frcnn_common.h"
#include "frcnn_layout.h"
#include "eval_dev.h"
FRCNN_LAYOUT_STAMP(coco_eval_pooled);

#define POOL_A 4                        // area ranges: all, small, medium, large
#define POOL_CHUNK 256                  // ranked detections staged in LDS at a time by a chain
#define POOL_PER_THREAD (EVAL_MAX_G / EVAL_THREADS)
#define POOL_F_IGNORED 1u               // a chain's ground-truth flags
#define POOL_F_CROWD 2u

// the carving of the workspace behind its 256-byte aligned base, as the kernels address it (pool_ws_layout is the host's side of it)
#define POOL_OFF_GPERM 256                                                     // int32 [EVAL_MAX_G]: pooled index -> original position
#define POOL_OFF_DOUT (POOL_OFF_GPERM + EVAL_MAX_G * 4)                        // u8 [EVAL_MAX_P]: bit a = the detection's area lies outside range a
#define POOL_OFF_DET (POOL_OFF_DOUT + EVAL_MAX_P)                              // double [5][EVAL_MAX_P]: x, y, x + w, y + h, w * h by rank
#define POOL_OFF_KEYS (POOL_OFF_DET + 5 * EVAL_MAX_P * 8)                      // u64 [D]
static_assert(POOL_OFF_DET % 8 == 0 && POOL_OFF_KEYS % 256 == 0, "pooled workspace: misaligned carving");
static_assert(EVAL_MAX_G % EVAL_THREADS == 0 && EVAL_MAX_G <= 65536 && EVAL_MAX_C * EVAL_MAX_P <= (1 << 20) && EVAL_MAX_C <= 256, "pooled keys: field widths");

struct PoolHeader {                     // written by the rank kernel, read by every chain
    int32_t nd;                         // ranked detections (0: nothing to match, or a frame with an error)
    int32_t ng;                         // ground truths
    u64 base;                           // the frame's first record slot
};

struct PoolWs { char *base; size_t total; };

// The fixed pieces (header | gperm | dout | det) are ONE piece of the carver, POOL_OFF_KEYS bytes: the keys behind it then lie where
// the kernels' POOL_OFF_KEYS says (a multiple of 256, asserted above), and the size cannot move away from the offsets.
static PoolWs pool_ws_layout(int64_t D, void *workspace)
{
    PoolWs w;
    WsCarver c = WsCarver::any_base(workspace);
    w.base = (char *)c.take(POOL_OFF_KEYS);
    c.get<u64>((size_t)D);
    w.total = c.bytes();
    return w;
}

size_t frcnn_ws_coco_eval_pooled(int64_t D, int64_t G) { return eval_supported(D, G) ? pool_ws_layout(D, nullptr).total : 0; }

__device__ __forceinline__ bool pool_outside(double area, int a)
{
    const double lo = a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0);               // [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10]
    const double hi = a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10);
    return area < lo || area > hi;
}

// Bitonic network over s[0 .. n2) in LDS, n2 a power of two, descending.  Every thread of the workgroup calls it, after a barrier; it ends
// with one.
__device__ __forceinline__ void pool_sort_desc(u64 *s, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += EVAL_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 x = s[i], y = s[l];
                    if ((i & k) == 0 ? x < y : x > y) { s[i] = y; s[l] = x; }
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(EVAL_THREADS) void coco_pooled_rank_kernel(
    const float4 *__restrict__ boxes, const int32_t *__restrict__ labels, const float *__restrict__ scores, const int32_t *__restrict__ count_dev,
    int D, const double *__restrict__ gt_area, const int32_t *__restrict__ gt_labels, const uint8_t *__restrict__ gt_crowd,
    const int32_t *__restrict__ n_gt_dev, int G, const int32_t *__restrict__ frame, int nc, int max_det, u64 *__restrict__ npig,
    float *__restrict__ rec_score, int32_t *__restrict__ rec_label, int32_t *__restrict__ rec_image, int32_t *__restrict__ rec_rank,
    uint32_t *__restrict__ rec_flags, long long rec_cap, u64 *__restrict__ cursor, int32_t *__restrict__ err, char *__restrict__ ws)
{
    __shared__ u64 s_key[EVAL_MAX_P];
    __shared__ int s_hist[256];
    __shared__ int s_np[POOL_A];
    __shared__ int s_bad, s_fill, s_sel, s_rem;
    __shared__ u64 s_base;
    PoolHeader *hdr = (PoolHeader *)ws;
    int32_t *gperm = (int32_t *)(ws + POOL_OFF_GPERM);
    uint8_t *dout = (uint8_t *)(ws + POOL_OFF_DOUT);
    double *det = (double *)(ws + POOL_OFF_DET);
    u64 *keys = (u64 *)(ws + POOL_OFF_KEYS);
    const int tid = threadIdx.x;
    const int cnt_raw = *count_dev, ng_raw = *n_gt_dev;
    int e = eval_frame_error(cnt_raw, D, ng_raw, G);
    const int n = e ? 0 : cnt_raw;
    const int ng = e ? 0 : (ng_raw < 0 ? 0 : ng_raw);
    if (tid == 0) { s_bad = 0; s_fill = 0; s_base = 0ull; }
    if (tid < POOL_A) s_np[tid] = 0;
    __syncthreads();
    {
        int bad = 0;
        for (int i = tid; i < n; i += EVAL_THREADS) {
            const int l = labels[i];
            if (l < 0 || l >= nc) bad = 1;
        }
        for (int g = tid; g < ng; g += EVAL_THREADS) {
            const int l = gt_labels[g];
            if (l < 0 || l >= nc) bad = 1;
        }
        if (bad) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) e |= EVAL_ERR_LABEL_RANGE;
    // a frame that reports an error is not recorded at all (eval_dev.h)
    if (e) {
        if (tid == 0) {
            atomicOr(err, e);
            hdr->nd = 0; hdr->ng = 0; hdr->base = 0ull;
        }
        return;
    }
    // ---- the ground truths' pooled order (label ascending, position ascending), and npig
    int g2 = 1;
    while (g2 < ng) g2 <<= 1;
    for (int i = tid; i < g2; i += EVAL_THREADS) s_key[i] = i < ng ? ~(((u64)(uint32_t)gt_labels[i] << 16) | (u64)i) : 0ull;     // padding sorts last
    __syncthreads();
    pool_sort_desc(s_key, g2);
    {
        int c[POOL_A] = {0, 0, 0, 0};
        for (int p = tid; p < ng; p += EVAL_THREADS) {
            const int g = (int)(~s_key[p] & 0xffffull);
            gperm[p] = g;
            const bool crowd = gt_crowd[g] != 0;
            const double ar = gt_area[g];
#pragma unroll
            for (int a = 0; a < POOL_A; ++a) c[a] += !(crowd || pool_outside(ar, a));                   // gtIg = iscrowd or area outside the range
        }
#pragma unroll
        for (int a = 0; a < POOL_A; ++a)
            if (c[a]) atomicAdd(&s_np[a], c[a]);
    }
    __syncthreads();                                                                                    // s_key is free again
    if (tid < POOL_A && s_np[tid]) atomicAdd(&npig[tid], (u64)s_np[tid]);
    // ---- the max_det first detections in (score descending, label ascending, position ascending)
    const int nd = n < max_det ? n : max_det;
    int d2 = 1;
    while (d2 < nd) d2 <<= 1;
    if (n <= max_det) {
        for (int i = tid; i < d2; i += EVAL_THREADS)
            s_key[i] = i < n ? ((u64)eval_orderable(scores[i]) << 32) | (u64)(0xffffffffu - (((uint32_t)labels[i] << 20) | (uint32_t)i)) : 0ull;
    } else {
        for (int i = tid; i < n; i += EVAL_THREADS)
            keys[i] = ((u64)eval_orderable(scores[i]) << 32) | (u64)(0xffffffffu - (((uint32_t)labels[i] << 20) | (uint32_t)i));
        __syncthreads();
        // radix select, 8 bits at a time from the top: `prefix` becomes the nd-th largest key
        u64 prefix = 0;
        int remaining = nd;
        for (int shift = 56; shift >= 0; shift -= 8) {
            s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += EVAL_THREADS) {
                const u64 key = keys[i];
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
        for (int i = tid; i < n; i += EVAL_THREADS) {
            const u64 key = keys[i];
            if (key >= prefix) {                                                                        // exactly nd of them: the keys are distinct
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < nd) s_key[slot] = key;
            }
        }
        for (int i = nd + tid; i < d2; i += EVAL_THREADS) s_key[i] = 0ull;
    }
    __syncthreads();
    pool_sort_desc(s_key, d2);
    // ---- the records, with zeroed flag words, and the ranked boxes for the chains
    if (tid == 0) {
        if (nd > 0) s_base = atomicAdd(cursor, (u64)nd);                                                // a full store keeps counting: summarize() reports the loss
        hdr->nd = nd; hdr->ng = ng; hdr->base = s_base;
    }
    __syncthreads();
    const u64 base = s_base;
    const float fw = (float)frame[0], fh = (float)frame[1];
    const int image_id = frame[2];
    for (int r = tid; r < nd; r += EVAL_THREADS) {
        const int i = (int)((0xffffffffu - (uint32_t)s_key[r]) & 0xfffffu);
        const float4 b = boxes[i];
        const float X1 = b.x * fw, Y1 = b.y * fh, X2 = b.z * fw, Y2 = b.w * fh;                         // test.py:70-71, in fp32
        const float Wf = X2 - X1, Hf = Y2 - Y1;                                                         // convert_to_xywh, in fp32
        const double dx = (double)X1, dy = (double)Y1, dw = (double)Wf, dh = (double)Hf;                // .tolist()
        const double area = dw * dh;
        det[r] = dx; det[EVAL_MAX_P + r] = dy; det[2 * EVAL_MAX_P + r] = dx + dw; det[3 * EVAL_MAX_P + r] = dy + dh; det[4 * EVAL_MAX_P + r] = area;
        uint32_t o = 0;
#pragma unroll
        for (int a = 0; a < POOL_A; ++a)
            if (pool_outside(area, a)) o |= 1u << a;
        dout[r] = (uint8_t)o;
        const u64 slot = base + (u64)r;
        if (slot < (u64)rec_cap) {
            rec_score[slot] = scores[i];
            rec_label[slot] = 0;
            rec_image[slot] = image_id;
            rec_rank[slot] = r;
#pragma unroll
            for (int a = 0; a < POOL_A; ++a) rec_flags[slot * POOL_A + a] = 0u;
        }
    }
}

// The walk's decision for one detection as the maximum of one key per ground truth: (POOL_K_VALID | POOL_K_NOT_IGNORED | the IoU's bits,
// pooled index), compared as a pair.  An IoU lies in [0, 2), so its float64 bits are below 2^62 and ascend with it: the key orders first
// "not ignored" (evaluateImg looks at the ignored ones only when none of the others matched), then the IoU, then the pooled index
// ("< best: continue" keeps the LAST of equal IoUs).  No candidate is (0, -1), below every key.
#define POOL_K_VALID (1ull << 63)
#define POOL_K_NOT_IGNORED (1ull << 62)
__device__ __forceinline__ void pool_take(u64 &bk, int &bi, u64 k, int i)
{
    if (k > bk || (k == bk && i > bi)) { bk = k; bi = i; }
}
// One step of the DPP chain of frcnn_dev.h's wave_reduce_dpp for the pair: a lane without a source combines with (0, -1).
template <int CTRL, int RMASK> __device__ __forceinline__ void pool_dpp_step(u64 &k, int &i)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, RMASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, RMASK, 0xf, false);
    const int oi = __builtin_amdgcn_update_dpp(-1, i, CTRL, RMASK, 0xf, false);
    pool_take(k, i, ((u64)hi << 32) | (u64)lo, oi);
}
// every lane active; lane 63 ends with the wave's maximum
__device__ __forceinline__ void pool_wave_max(u64 &k, int &i)
{
    pool_dpp_step<0x111, 0xf>(k, i);    // row_shr:1
    pool_dpp_step<0x112, 0xf>(k, i);    // row_shr:2
    pool_dpp_step<0x114, 0xf>(k, i);    // row_shr:4
    pool_dpp_step<0x118, 0xf>(k, i);    // row_shr:8   -> lane 15 of every row holds the row's result
    pool_dpp_step<0x142, 0xa>(k, i);    // row_bcast:15 into rows 1 and 3
    pool_dpp_step<0x143, 0xc>(k, i);    // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's result
}

__global__ __launch_bounds__(EVAL_THREADS) void coco_pooled_match_kernel(
    const double *__restrict__ gt_boxes, const double *__restrict__ gt_area, const uint8_t *__restrict__ gt_crowd,
    const double *__restrict__ thr_dev, int T, uint32_t *__restrict__ rec_flags, long long rec_cap, const char *__restrict__ ws)
{
    __shared__ double s_d[5][POOL_CHUNK];
    __shared__ uint8_t s_do[POOL_CHUNK];
    __shared__ uint8_t s_code[EVAL_MAX_P];
    __shared__ u64 s_rk[2][EVAL_THREADS / 64];                  // [parity of the step][wave]: the waves' maxima
    __shared__ int s_ri[2][EVAL_THREADS / 64];
    const PoolHeader *hdr = (const PoolHeader *)ws;
    const int32_t *gperm = (const int32_t *)(ws + POOL_OFF_GPERM);
    const uint8_t *dout = (const uint8_t *)(ws + POOL_OFF_DOUT);
    const double *det = (const double *)(ws + POOL_OFF_DET);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int a = blockIdx.x / T, t = blockIdx.x % T;
    const int nd = hdr->nd, ng = hdr->ng;
    if (nd <= 0) return;
    const u64 base = hdr->base;
    // ---- this thread's ground truths: pooled index tid + 256 i
    double gx[POOL_PER_THREAD], gy[POOL_PER_THREAD], gxe[POOL_PER_THREAD], gye[POOL_PER_THREAD], gwh[POOL_PER_THREAD];
    uint32_t gf[POOL_PER_THREAD];
#pragma unroll
    for (int i = 0; i < POOL_PER_THREAD; ++i) {
        const int p = tid + EVAL_THREADS * i;
        gx[i] = gy[i] = gxe[i] = gye[i] = gwh[i] = 0.0;
        gf[i] = 0u;
        if (p < ng) {
            const int g = gperm[p];
            const double x = gt_boxes[4 * g], y = gt_boxes[4 * g + 1], w = gt_boxes[4 * g + 2], h = gt_boxes[4 * g + 3];
            const bool crowd = gt_crowd[g] != 0;
            gx[i] = x; gy[i] = y; gxe[i] = x + w; gye[i] = y + h; gwh[i] = w * h;
            gf[i] = (crowd ? POOL_F_CROWD : 0u) | ((crowd || pool_outside(gt_area[g], a)) ? POOL_F_IGNORED : 0u);
        }
    }
    uint32_t matched = 0u;
    const double thr = thr_dev[t];
    const double best0 = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;                                          // min([t, 1 - 1e-10])
    // A wave all of whose ground truths lie behind ng (wave-uniform) has no candidate in any step: it leaves (0, -1) in both of its
    // words once, keeps the barriers and nothing else.  Wave 0 always works: its thread 0 writes the codes.
    const bool busy = wv == 0 || wv * 64 < ng;
    if (!busy && lane == 63) { s_rk[0][wv] = 0ull; s_ri[0][wv] = -1; s_rk[1][wv] = 0ull; s_ri[1][wv] = -1; }
    for (int d = 0; d < nd; ++d) {
        const int c = d & (POOL_CHUNK - 1);
        if (c == 0) {
            __syncthreads();                                                                            // the chunk before it has been read
            if (d + tid < nd) {
#pragma unroll
                for (int f = 0; f < 5; ++f) s_d[f][tid] = det[f * EVAL_MAX_P + d + tid];
                s_do[tid] = dout[d + tid];
            }
            __syncthreads();
        }
        const int par = d & 1;
        if (busy) {
            const double dx = s_d[0][c], dy = s_d[1][c], dxe = s_d[2][c], dye = s_d[3][c], dwh = s_d[4][c];
            u64 k = 0ull;
            int m = -1;
#pragma unroll
            for (int i = 0; i < POOL_PER_THREAD; ++i) {
                const int p = tid + EVAL_THREADS * i;
                const bool crowd = (gf[i] & POOL_F_CROWD) != 0u;
                if (p >= ng || (((matched >> i) & 1u) && !crowd)) continue;
                double iou = 0.0;
                const double w = fmin(dxe, gxe[i]) - fmax(dx, gx[i]);
                if (!(w <= 0.0)) {
                    const double h = fmin(dye, gye[i]) - fmax(dy, gy[i]);
                    if (!(h <= 0.0)) {
                        const double in = w * h;
                        const double u = crowd ? dwh : dwh + gwh[i] - in;
                        iou = in / u;
                    }
                }
                if (!(iou >= best0)) continue;
                pool_take(k, m, POOL_K_VALID | ((gf[i] & POOL_F_IGNORED) ? 0ull : POOL_K_NOT_IGNORED) | (u64)__double_as_longlong(iou), p);
            }
            pool_wave_max(k, m);
            if (lane == 63) { s_rk[par][wv] = k; s_ri[par][wv] = m; }
        }
        __syncthreads();
        if (busy) {
            u64 k = 0ull;
            int mm = -1;
#pragma unroll
            for (int w = 0; w < EVAL_THREADS / 64; ++w) pool_take(k, mm, s_rk[par][w], s_ri[par][w]);
            if (mm >= 0 && (mm & (EVAL_THREADS - 1)) == tid) matched |= 1u << (mm / EVAL_THREADS);
            if (tid == 0) {
                uint32_t code;
                if (mm >= 0) code = (k & POOL_K_NOT_IGNORED) ? FRCNN_EVAL_TP : FRCNN_EVAL_IGNORED;
                else code = ((s_do[c] >> a) & 1u) ? FRCNN_EVAL_IGNORED : FRCNN_EVAL_FP;
                s_code[d] = (uint8_t)code;
            }
        }
    }
    __syncthreads();
    for (int d = tid; d < nd; d += EVAL_THREADS) {
        const u64 slot = base + (u64)d;
        if (slot < (u64)rec_cap) atomicOr(&rec_flags[slot * POOL_A + a], (uint32_t)s_code[d] << (2 * t));
    }
}

FRCNN_EXPORT int frcnn_coco_eval_update_pooled(const float *boxes, const int32_t *labels, const float *scores, const int32_t *count_dev,
                                               int64_t det_capacity, const double *gt_boxes, const double *gt_area, const int32_t *gt_labels,
                                               const uint8_t *gt_iscrowd, const int32_t *n_gt_dev, int64_t gt_capacity, const int32_t *frame_dev,
                                               const double *thresholds_dev, int T, int C, int max_det, int64_t *npig, float *rec_score,
                                               int32_t *rec_label, int32_t *rec_image, int32_t *rec_rank, uint32_t *rec_flags,
                                               int64_t record_capacity, int64_t *cursor, int32_t *error_word, void *workspace,
                                               size_t workspace_bytes, void *stream)
{
    if (C < 2 || C > EVAL_MAX_C || T < 1 || T > EVAL_MAX_T || max_det < 1 || max_det > EVAL_MAX_P || !eval_supported(det_capacity, gt_capacity) ||
        det_capacity > (int64_t)(C - 1) * EVAL_MAX_P)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED,
                               "coco_eval_update_pooled: C = %d, T = %d, max_det = %d, detection capacity %lld, ground-truth capacity %lld outside "
                               "2 <= C <= %d, 1 <= T <= %d, 1 <= max_det <= %d, 1 <= D <= (C-1) * %d, 1 <= G <= %d", C, T, max_det,
                               (long long)det_capacity, (long long)gt_capacity, EVAL_MAX_C, EVAL_MAX_T, EVAL_MAX_P, EVAL_MAX_P, EVAL_MAX_G);
    FRCNN_REQUIRE(boxes && labels && scores && count_dev && gt_boxes && gt_area && gt_labels && gt_iscrowd && n_gt_dev && frame_dev && thresholds_dev &&
                  npig && rec_score && rec_label && rec_image && rec_rank && rec_flags && cursor && error_word && workspace,
                  "coco_eval_update_pooled: NULL pointer");
    FRCNN_REQUIRE(record_capacity >= 1, "coco_eval_update_pooled: record_capacity must be >= 1");
    FRCNN_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)gt_boxes & 7) == 0 && ((uintptr_t)gt_area & 7) == 0,
                  "coco_eval_update_pooled: boxes must be 16-byte aligned, gt_boxes and gt_area 8-byte aligned");
    const PoolWs w = pool_ws_layout(det_capacity, workspace);
    FRCNN_REQUIRE_WS("coco_eval_update_pooled", workspace_bytes, w.total);
    char *ws = w.base;
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(coco_pooled_rank_kernel, dim3(1), dim3(EVAL_THREADS), 0, s, (const float4 *)boxes, labels, scores, count_dev, (int)det_capacity,
                 gt_area, gt_labels, gt_iscrowd, n_gt_dev, (int)gt_capacity, frame_dev, C - 1, max_det, (u64 *)npig, rec_score, rec_label, rec_image,
                 rec_rank, rec_flags, (long long)record_capacity, (u64 *)cursor, error_word, ws);
    FRCNN_CHECK_LAUNCH("coco_pooled_rank_kernel");
    FRCNN_LAUNCH(coco_pooled_match_kernel, dim3((unsigned)(POOL_A * T)), dim3(EVAL_THREADS), 0, s, gt_boxes, gt_area, gt_iscrowd, thresholds_dev, T,
                 rec_flags, (long long)record_capacity, (const char *)ws);
    FRCNN_CHECK_LAUNCH("coco_pooled_match_kernel");
    return FRCNN_OK;
}
