/*
 * frcnn_hip.h -- C ABI of libfrcnn_hip.so: the MI355X (gfx950) Faster R-CNN
 * proposal / RoI-head hot path.
 *
 * The reference (csm-kr/faster_rcnn_pytorch) is pure Python and has no FFI; its
 * boundary for this path is the Python call surface of models/model.py + anchor.py
 * and, beneath it, five torchvision entry points.  Every function below names the
 * reference interface (file:line under /root/reference) it replaces; the ctypes
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - extern "C"; plain pointers and sizes; no torch types.  Returns 0 on success,
 *    a negative frcnn_status otherwise; never throws, never allocates device
 *    memory, never synchronises the stream (unless stated).
 *  - Every pointer is a DEVICE pointer unless the name ends in _host.  The caller
 *    owns every buffer, workspaces included.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *  - Variable-length results use a fixed-capacity buffer + a device-side int32
 *    count, so a whole training step can be enqueued without a host round trip.
 *  - Boxes are fp32 xyxy, normalised to [0,1] by image (w,h) unless stated;
 *    indices are int64 (torch.long in the reference), argmax is int32.
 *  - Arithmetic is IEEE binary32 with no FMA contraction (the reference's eager
 *    op chains round after every op); exp / log2 are the fixed +-*-/ sequences
 *    restated in oracle/frcnn_oracle.c, so integer results (sort order, NMS keep
 *    lists, level ids, labels) are bit-exact against the oracle.
 */
#ifndef FRCNN_HIP_H
#define FRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRCNN_ABI_VERSION 7

typedef enum {
    FRCNN_OK = 0,
    FRCNN_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, K > capacity ... */
    FRCNN_ERR_UNSUPPORTED = -2,   /* size outside what the kernels are built for */
    FRCNN_ERR_WORKSPACE = -3,     /* workspace too small (see frcnn_workspace_bytes) */
    FRCNN_ERR_LAUNCH = -4         /* hipGetLastError() after a launch was not hipSuccess */
} frcnn_status;

typedef enum { FRCNN_DTYPE_F32 = 0, FRCNN_DTYPE_BF16 = 1 } frcnn_dtype;

/* operation ids for frcnn_workspace_bytes() */
typedef enum {
    FRCNN_OP_TOPK = 1,            /* n1 = N candidates */
    FRCNN_OP_NMS = 2,             /* n1 = K boxes */
    FRCNN_OP_REGION_PROPOSAL = 3, /* n1 = N anchors, n2 = K */
    FRCNN_OP_RPN_TARGETS = 4,     /* n1 = N anchors, n2 = G */
    FRCNN_OP_HEAD_TARGETS = 5,    /* n1 = P + G candidates */
    FRCNN_OP_PREPROCESS = 6,      /* n1 = (h << 32) | w of the source frame, n2 = (oh << 32) | ow of the resized frame */
    FRCNN_OP_HEAD_BWD = 7,        /* n1 = C (frcnn_rpn_head_tail_ml_bwd) */
    FRCNN_OP_RPN_CONV = 8,        /* frcnn_rpn_conv_head_fwd / frcnn_rpn_conv_bwd_data (packed bf16 weights) */
    FRCNN_OP_RPN_CONV_WGRAD = 9,  /* frcnn_rpn_conv_wgrad (per-split partial gradients) */
    FRCNN_OP_RPN_CONV_F32 = 10,   /* n1 = C: frcnn_rpn_conv3x3_f32_fwd / _bwd_data / _wgrad (ticket words, transposed weights, slabs) */
    FRCNN_OP_DETECT = 11,         /* n1 = P RoI rows, n2 = C classes: frcnn_detect_postprocess (0 outside its limits) */
    FRCNN_OP_EVAL = 12,           /* n1 = detection capacity, n2 = ground-truth capacity: frcnn_eval_update (0 outside its limits) */
    FRCNN_OP_COCO_EVAL = 13,      /* n1 = detection capacity, n2 = ground-truth capacity: frcnn_coco_eval_update (0 outside its limits) */
    FRCNN_OP_EVAL_MERGE = 14,     /* n1 = W * shard record capacity, n2 = W * shard image capacity: frcnn_eval_merge (0 outside its limits) */
    FRCNN_OP_COCO_EVAL_POOLED = 15, /* n1 = detection capacity, n2 = ground-truth capacity: frcnn_coco_eval_update_pooled (0 outside its limits) */
    FRCNN_OP_DETECT_MERGE = 16    /* n1 = out_capacity, n2 = C classes: frcnn_detect_merge (0 outside its limits) */
} frcnn_op;

/* FRCNN_ABI_VERSION, or FRCNN_ERR_UNSUPPORTED (message in frcnn_last_error) when the objects the library was linked from were compiled
 * against different versions of its internal headers (a stale object; csrc/frcnn_layout.h): a binding must refuse such a library. */
int frcnn_abi_version(void);
/* The same check by itself (FRCNN_OK / FRCNN_ERR_UNSUPPORTED), and the stamp api.o was compiled with: a 64-bit hash of the sizes, field
 * offsets and constants of every structure two translation units share by layout (AnchorDesc, the sample sort's control block + plan). */
int frcnn_layout_check(void);
uint64_t frcnn_layout_stamp(void);
/* thread-local description of the last non-zero status returned on this thread */
const char *frcnn_last_error(void);
size_t frcnn_workspace_bytes(int op, int64_t n1, int64_t n2);

/* ---- anchors -------------------------------------------------------------------------------- */
/* FRCNNAnchorMaker.generate_anchor_base (anchor.py:15-32).  Host computation (done once).       */
int frcnn_anchor_base_host(int base_size, const double *ratios_host, int n_ratios,
                           const double *scales_host, int n_scales, float *out_host /*[nr*ns,4]*/);
/* torchvision AnchorGenerator.generate_anchors for ONE size (models/new_model.py:23-25). Host.  */
int frcnn_tv_base_anchors_host(float size, const float *ratios_host, int n_ratios, float *out_host /*[nr,4]*/);

/* Anchor grid over n_levels feature maps, level-major, position-major (y, x), base-minor:
 *   out[off_l + (y*fw_l + x)*A + a] = (base_l[a] + (x*sw_l, y*sh_l, x*sw_l, y*sh_l)) / (div_w, div_h, div_w, div_h)
 * One level, A = 9, stride 16, div = (W,H)  == FRCNNAnchorMaker._enumerate_shifted_anchor (anchor.py:34-55);
 * five levels, A = 3, strides (H//fh, W//fw) == AnchorGenerator(...)(ImageList, feats) followed by the
 * in-place division at models/new_model.py:46-47.  base_host: [n_levels, A, 4].  div = 1 -> pixels. */
int frcnn_anchor_grid(int n_levels, const int *fh_host, const int *fw_host,
                      const int *stride_h_host, const int *stride_w_host,
                      const float *base_host, int A, float div_w, float div_h,
                      float *out /*[N,4]*/, int64_t N, void *stream);

/* ---- box codec (utils/util.py:15-50) ---------------------------------------------------------- */
/* op: 0 xy_to_cxcy(a) | 1 cxcy_to_xy(a) | 2 decode(a = tcxcy, b = center_anchor) | 3 encode(a = gt_cxcy, b = anc_cxcy) */
int frcnn_box_codec(int op, const float *a, const float *b, int64_t n, float *out, void *stream);

/* find_jaccard_overlap (utils/util.py:66-102; eps = 1e-5) / box_iou (util/box_ops.py:24-37; eps = 0). */
int frcnn_pairwise_iou(const float *set1, int64_t n1, const float *set2, int64_t n2, float eps,
                       float *out /*[n1,n2]*/, void *stream);

/* ---- RegionProposal.forward (models/model.py:12-58, models/new_model.py:49-86) ------------------ */
/* Stage 1: fg softmax + decode + clamp + min-size filter (model.py:20-41).
 * anchors == NULL is not allowed here; see frcnn_region_proposal for the fused anchor-free form.
 * out_scores[i] = softmax(cls[i])[1], or -1 where (w < min_size_norm or h < min_size_norm).       */
int frcnn_proposal_prologue(const float *reg /*[N,4]*/, const float *cls /*[N,2]*/, const float *anchors /*[N,4]*/,
                            int64_t N, float min_size_norm, float *out_boxes /*[N,4]*/, float *out_scores /*[N]*/,
                            void *stream);

/* Stage 2: scores.sort(descending=True)[:K] (model.py:44-49).  Ties are ordered by ascending index
 * (torch's sort is unstable).  Only LIVE entries, score >= 0, are sorted: -0.0 and denormals are live,
 * negatives and NaNs of either sign are not and never appear.  out_count = min(K, #live), and exactly the first
 * out_count entries of the outputs are written.  The order is the total order on the score's bit pattern: every
 * +0.0 comes before any -0.0 (torch compares them equal: unpinned there).
 * boxes_in/out_boxes may both be NULL (no gather).                                                 */
int frcnn_topk_sorted(const float *scores /*[N]*/, const float *boxes_in /*[N,4] or NULL*/, int64_t N, int64_t K,
                      int64_t *out_idx /*[K]*/, float *out_scores /*[K]*/, float *out_boxes /*[K,4] or NULL*/,
                      int32_t *out_count, void *workspace, size_t workspace_bytes, void *stream);

/* Full descending argsort (every score live, negatives included): the sort inside torchvision.ops.nms
 * when the caller's boxes are not pre-sorted (per-class NMS, models/model.py:394).  Ties: ascending index.
 * Total order on the bit pattern: -0.0 < +0.0; a NaN with the sign bit clear sorts in front of +inf (larger
 * payload first), one with the sign bit set behind -inf (torch.sort puts every NaN first).                */
int frcnn_argsort_desc(const float *scores /*[N]*/, const float *boxes_in /*[N,4] or NULL*/, int64_t N,
                       int64_t *out_idx /*[N]*/, float *out_scores /*[N]*/, float *out_boxes /*[N,4] or NULL*/,
                       int32_t *out_count, void *workspace, size_t workspace_bytes, void *stream);

/* Stage 3: torchvision.ops.nms (model.py:53,394) on boxes already in visiting (score-descending) order.
 * Greedy, suppress when inter/(area_i+area_j-inter) > thr (strict).  Writes the first post_k kept
 * positions (ascending) to out_keep, their boxes to out_rois (optional) and the number to out_count.
 * n_boxes_dev (optional) is a device int32 with the live box count (<= K), e.g. frcnn_topk_sorted's count. */
int frcnn_nms(const float *boxes /*[K,4]*/, const int32_t *n_boxes_dev, int64_t K, float iou_threshold, int64_t post_k,
              int64_t *out_keep /*[post_k]*/, float *out_rois /*[post_k,4] or NULL*/, int32_t *out_count,
              void *workspace, size_t workspace_bytes, void *stream);

/* Per-class NMS of FRCNN._suppress (models/model.py:382-402; torchvision batched_nms semantics) in ONE launch pair
 * instead of C-1 nms calls + C-1 device-to-host copies: like frcnn_nms, but box j is suppressed only by a kept box i
 * with cls[i] == cls[j].  boxes / cls are in visiting (score-descending) order.                                      */
int frcnn_nms_classed(const float *boxes /*[K,4]*/, const int32_t *cls /*[K]*/, const int32_t *n_boxes_dev, int64_t K,
                      float iou_threshold, int64_t post_k, int64_t *out_keep, float *out_rois /*or NULL*/, int32_t *out_count,
                      void *workspace, size_t workspace_bytes, void *stream);

/* All of RegionProposal.forward in one call (prologue -> top-K -> NMS -> first P), no host sync.
 * anchors may be NULL when the single-level grid description is given (fh,fw,stride,base9x4 on host):
 * the anchors are then regenerated in registers and never read from HBM (anchor.py:34-55 fused away).
 * nms_level_offsets_host == NULL (default): ONE class-agnostic NMS over the K boxes of all levels -- what the reference does
 *   (models/new_model.py:74-83).
 * nms_level_offsets_host = [n_nms_levels + 1] anchor offsets (level l owns anchors [off[l], off[l+1])): the OPTIONAL per-FPN-level
 *   variant of BASELINE.json configs[3]: after the same global top-K, box j is suppressed only by a kept box of ITS OWN level
 *   (torchvision's RPN batched_nms over level ids), then the first P in score order.  n_nms_levels <= 8.                        */
int frcnn_region_proposal(const float *reg, const float *cls, const float *anchors /*[N,4] or NULL*/, int64_t N,
                          int fh, int fw, int stride, const float *base_host /*[A,4] or NULL*/, int A,
                          float div_w, float div_h,
                          float min_size_norm, int64_t pre_nms_top_k, float iou_threshold, int64_t post_nms_top_k,
                          const int64_t *nms_level_offsets_host /*[n_nms_levels + 1] or NULL*/, int n_nms_levels,
                          float *out_rois /*[P,4]*/, int32_t *out_count,
                          int64_t *out_src_idx /*[P] anchor index of each roi, or NULL*/,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- RPN head tail (models/model.py:79-83; models/new_model.py:109-113) ---------------------------------------- */
/* conv_raw [C,P] = the 3x3 inter_layer convolution WITHOUT its bias (NCHW, P = fh*fw).  Computes
 *   h = relu(conv_raw + b3);  cls = w_cls[n_cls,C] h + b_cls;  reg = w_reg[n_reg,C] h + b_reg
 * on the fp32 matrix cores and stores them as [P, n_cls] / [P, n_reg] row-major, i.e. exactly
 * pred.permute(0,2,3,1).contiguous().view(1,-1,2|4).  C % 64 == 0, n_cls + n_reg <= 64.                          */
int frcnn_rpn_head_tail_fwd(const float *conv_raw, int C, int64_t P, const float *b3,
                            const float *w_cls, const float *b_cls, int n_cls,
                            const float *w_reg, const float *b_reg, int n_reg,
                            float *out_cls, float *out_reg, void *stream);
/* The same for all FPN levels in one launch (models/new_model.py:37-44: the shared head applied per level, outputs
 * concatenated along the anchor axis).  conv_raw_levels / P_levels: HOST arrays (n_levels <= 5) of device pointers
 * [C, P_l] and position counts.  dtype: element type of the conv outputs (FRCNN_DTYPE_F32 | FRCNN_DTYPE_BF16);
 * mfma: FRCNN_DTYPE_F32 = exact fp32 contraction, FRCNN_DTYPE_BF16 = operands rounded to bf16, fp32 accumulate (the
 * mixed-precision configuration of BASELINE.json configs[4]; biases, outputs and everything downstream stay fp32). */
int frcnn_rpn_head_tail_ml_fwd(const void *const *conv_raw_levels, int dtype, int mfma, int C, const int64_t *P_levels, int n_levels,
                               const float *b3, const float *w_cls, const float *b_cls, int n_cls, const float *w_reg,
                               const float *b_reg, int n_reg, float *out_cls, float *out_reg, void *stream);

/* Backward of frcnn_rpn_head_tail_ml_fwd (what autograd derives from models/model.py:79-83 / new_model.py:109-113): given the
 * gradients of the two outputs (g_cls [sum P_l, n_cls], g_reg [sum P_l, n_reg], the outputs' own layout) it writes
 *   d_raw_levels[l] [C, P_l]  gradient of the bias-free 3x3 output (same dtype as conv_raw_levels: 0 = f32, 1 = bf16),
 *   dw_cls [n_cls, C], db_cls [n_cls], dw_reg [n_reg, C], db_reg [n_reg], db3 [C]  (fp32, fully overwritten).
 * C must be 256 or 512; workspace >= frcnn_workspace_bytes(FRCNN_OP_HEAD_BWD, C, 0).  Exact fp32 MFMA; sums in a fixed order. */
int frcnn_rpn_head_tail_ml_bwd(const void *const *conv_raw_levels, void *const *d_raw_levels, int dtype, int C, const int64_t *P_levels,
                               int n_levels, const float *b3, const float *w_cls, int n_cls, const float *w_reg, int n_reg,
                               const float *g_cls, const float *g_reg, float *dw_cls, float *db_cls, float *dw_reg, float *db_reg,
                               float *db3, void *workspace, size_t workspace_bytes, void *stream);

/* The whole FPN RPN head (models/new_model.py:89-114) in the bf16 mixed-precision configuration as one MFMA implicit-GEMM kernel:
 * 3x3 conv (256 -> 256, bf16 operands, fp32 accumulate) -> raw_levels (bf16, the bias-free conv output kept for backward) ->
 * bias + ReLU + both 1x1 heads -> out_cls [sum P_l, n_cls], out_reg [sum P_l, n_reg] (fp32, the layout of frcnn_rpn_head_tail_ml_fwd).
 * feat_levels / raw_levels: [256, H_l, W_l] bf16 NCHW; w3 [256,256,3,3], w_cls [n_cls,256], w_reg [n_reg,256], biases: fp32.
 * workspace >= frcnn_workspace_bytes(FRCNN_OP_RPN_CONV, 0, 0) (the weights re-packed to bf16 on every call). */
int frcnn_rpn_conv_head_fwd(const void *const *feat_levels_bf16, void *const *raw_levels_bf16, const int *H_host, const int *W_host, int n_levels,
                            int C, const float *w3, const float *b3, const float *w_cls, const float *b_cls, int n_cls, const float *w_reg,
                            const float *b_reg, int n_reg, float *out_cls, float *out_reg, void *workspace, size_t workspace_bytes, void *stream);

/* Backward-data of that 3x3 convolution (what autograd derives for `inter_layer`, models/new_model.py:96,109) on the same implicit-GEMM
 * kernel: d_feat[ci] = conv3x3(d_raw, W3 transposed and flipped), bf16 operands, fp32 accumulate, bf16 output.  d_raw_levels /
 * d_feat_levels: [256, H_l, W_l] bf16 NCHW.  workspace >= frcnn_workspace_bytes(FRCNN_OP_RPN_CONV, 0, 0).                         */
int frcnn_rpn_conv_bwd_data(const void *const *d_raw_levels_bf16, void *const *d_feat_levels_bf16, const int *H_host, const int *W_host, int n_levels,
                            int C, const float *w3, void *workspace, size_t workspace_bytes, void *stream);

/* Weight gradient of that convolution: dw3 [256,256,3,3] fp32 (fully overwritten) = sum over levels and positions of
 * d_raw[co](y, x) * feat[ci](y + ky - 1, x + kx - 1), bf16 operands, fp32 accumulate, split over the positions with a fixed-order
 * finalize (bit-reproducible).  workspace >= frcnn_workspace_bytes(FRCNN_OP_RPN_CONV_WGRAD, 0, 0).                                */
int frcnn_rpn_conv_wgrad(const void *const *feat_levels_bf16, const void *const *d_raw_levels_bf16, const int *H_host, const int *W_host, int n_levels,
                         int C, float *dw3, void *workspace, size_t workspace_bytes, void *stream);

/* The RPN head's 3x3 convolution in fp32 -- `self.inter_layer` of models/model.py:68-70,79 (512 -> 512 on the VGG16 map) and
 * models/new_model.py:96-98,109 (256 -> 256 on the FPN levels), WITHOUT its bias (frcnn_rpn_head_tail_* adds it) -- on
 * v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate, sums in a fixed order (bit-reproducible; a k-ordered fmaf chain per
 * output inside a K range, K ranges added in range order).  feat_levels / out_levels: [C, H_l, W_l] fp32 NCHW, batch 1; w3 [C, C, 3, 3]
 * in the reference's layout; C a multiple of 128.
 * The three calls share ONE workspace of frcnn_rpn_conv3x3_f32_workspace(H, W, n_levels, C) bytes that is DEDICATED to them and ZERO
 * before the first call (its ticket words are left zero by every call); calls on one workspace must be stream-ordered.
 *   _fwd      : out[co] = sum_ci conv3x3(feat[ci], w3[co][ci]), padding 1.
 *   _bwd_data : d_feat[ci] = sum_co conv3x3(d_out[co], w3[co][ci] flipped): what autograd derives for the input.
 *   _wgrad    : dw3[co][ci][ky][kx] = sum over levels and positions of d_out[co](y, x) * feat[ci](y + ky - 1, x + kx - 1) (fully overwritten). */
size_t frcnn_rpn_conv3x3_f32_workspace(const int *H_host, const int *W_host, int n_levels, int C);
int frcnn_rpn_conv3x3_f32_fwd(const float *const *feat_levels, float *const *out_levels, const int *H_host, const int *W_host, int n_levels, int C,
                              const float *w3, void *workspace, size_t workspace_bytes, void *stream);
int frcnn_rpn_conv3x3_f32_bwd_data(const float *const *d_out_levels, float *const *d_feat_levels, const int *H_host, const int *W_host, int n_levels,
                                   int C, const float *w3, void *workspace, size_t workspace_bytes, void *stream);
int frcnn_rpn_conv3x3_f32_wgrad(const float *const *feat_levels, const float *const *d_out_levels, const int *H_host, const int *W_host, int n_levels,
                                int C, float *dw3, void *workspace, size_t workspace_bytes, void *stream);

/* The same stage for the backbone's own 3x3 convolutions (padding 1, stride 1, batch 1, fp32): the layers the reference takes from torchvision --
 * `self.extractor = nn.Sequential(*list(vgg16.features)[:-1])` models/model.py:279-281 (conv3_x 256 channels on 150 x 250, conv4_x / conv5_x 512
 * channels on 75 x 125 / 37 x 62 at 600 x 1000) and the FPN's output convolutions behind models/new_model.py:372 (256 -> 256 on P2..P5) -- which
 * are 2/3 of the training step's GPU time through the vendor library.  w [Cout, Cin, 3, 3] in the reference's layout.
 *   _fwd      : y[co] = act(bias[co] + sum_ci conv3x3(x[ci], w[co][ci])); bias may be NULL; act = ReLU when relu != 0 (the Conv2d + ReLU(inplace)
 *               pair of vgg16.features in one pass).  Cin a multiple of 32, Cout a multiple of 64 (64-row GEMM tiles where a side is not a multiple of 128).
 *               relu_bits (optional, frcnn_conv3x3_f32_relu_bits_words(H, W, n_levels, Cout) uint16 words, caller-owned): the sign pattern of the
 *               ReLU outputs, one word per (channel, output tile) -- all the backward needs of them, at 1/32 of their bytes.
 *   _bwd_data : dx[ci] = sum_co conv3x3(g[co], w[co][ci] flipped), g = dy where the forward's relu_bits are set (autograd's threshold_backward
 *               folded into the input transform), or g = dy when relu_bits is NULL.  Cin a multiple of 64, Cout of 32.
 *   _wgrad    : dw[co][ci][ky][kx] = sum over levels and positions of g[co](y, x) * x[ci](y + ky - 1, x + kx - 1) (fully overwritten); dbias[co] =
 *               sum of g[co] (NULL: not wanted).  Cin and Cout multiples of 64.
 * Workspace: frcnn_conv3x3_f32_workspace(H, W, n_levels, Cin, Cout) bytes, the same DEDICATED zero-before-first-use block as the RPN calls
 * above (one block sized for the largest layer serves all of them; calls on it must be stream-ordered).  Bit-reproducible.                  */
size_t frcnn_conv3x3_f32_workspace(const int *H_host, const int *W_host, int n_levels, int Cin, int Cout);
/* x_transformed (optional, frcnn_conv3x3_f32_xt_floats(H, W, n_levels, Cin) floats, caller-owned): _fwd leaves the transformed activations
 * B^T d B there instead of in the scratch workspace, and a later _wgrad of the same layer given the same buffer skips transforming them
 * again -- 0.6 GB per VGG16 step on a 288 GB device for one launch less per layer.  NULL: scratch / transform again. */
size_t frcnn_conv3x3_f32_xt_floats(const int *H_host, const int *W_host, int n_levels, int Cin);
/* u_rotated (optional, frcnn_conv3x3_f32_u_floats floats, caller-owned): _fwd also leaves the transformed ROTATED weights there (same launch), and a later
 * _bwd_data of the same layer given the buffer starts without its weight transform.  NULL: _bwd_data transforms the weights itself. */
size_t frcnn_conv3x3_f32_u_floats(const int *H_host, const int *W_host, int n_levels, int Cin, int Cout);
/* dy_transformed (optional, frcnn_conv3x3_f32_xt_floats(H, W, n_levels, Cout) floats, caller-owned): _bwd_data stages the output gradient once and also writes
 * its weight-gradient transform A g A^T there (with want_bias_partials != 0 also the bias gradient's partial sums, in the workspace); a _wgrad of the same
 * layer called NEXT on the same workspace with that buffer skips its own pass over the gradient.  NULL: each call transforms the gradient itself. */
size_t frcnn_conv3x3_f32_relu_bits_words(const int *H_host, const int *W_host, int n_levels, int Cout);
/* relu = 2 (fwd): ReLU + max_pool2d(2, 2) (floor) in the output transform -- the MaxPool2d behind conv1_2 / conv2_2 / conv3_3 / conv4_3 of vgg16.features:
 * y_levels are then [Cout, H/2, W/2], the full-resolution activations are never written, and relu_bits holds per 2 x 2 window the position of the
 * maximum and whether it was positive.  The gradient calls take `pooled` = 1 with those words: dy_levels are [Cout, H/2, W/2] and max_pool2d's and the
 * ReLU's backward happen while the gradient is staged (H, W stay the convolution's own size everywhere).  Needs the 4 x 4 tile: frcnn_conv3x3_f32_tile_size
 * (2 or 4, the tile the calls will use for these shapes). */
int frcnn_conv3x3_f32_tile_size(const int *H_host, const int *W_host, int n_levels);
/* 1 when _fwd (and, with need_grads, _bwd_data and _wgrad) would accept these shapes, else 0: the question a caller's dispatch asks before routing a layer here. */
int frcnn_conv3x3_f32_supported(const int *H_host, const int *W_host, int n_levels, int Cin, int Cout, int need_grads);
/* What the three calls would execute for these shapes, from the host functions the launches themselves use; launches nothing (without a device: 256 CUs).
 * plan_host receives FRCNN_CONV_PLAN_INTS ints (plan_len >= that):
 *   head     [0] output tile size m (2 or 4)   [1] tile padding tg (64 or 128)   [2] padded tile total   [3] n_levels   [4] workgroup slots of the forward's /
 *            data gradient's product   [5] of the weight gradient's   [6] 1 when the pooled forms (relu = 2, pooled = 1) are available (m = 4)   [7] 0
 *   products three of FRCNN_CONV_PLAN_PRODUCT ints at FRCNN_CONV_PLAN_HEAD: forward, data gradient, weight gradient
 *            [0] 1 when the call accepts the shapes (else the rest is 0)   [1] product tile height   [2] width   [3] tiles along the channel side   [4] along the
 *            other side   [5] K chunks of 32   [6] n_tiles   [7] units = n_tiles x chunks   [8] G = workgroups launched   [9] schedule (FRCNN_CONV_SCHED_*)
 *   strips   two of FRCNN_CONV_PLAN_STRIPS ints behind the products: the transform launches over Cin channels (forward's input, the weight gradient's
 *            activations) and over Cout channels (the output gradient)
 *            [0] per_block the strips settled on   [1] strips per channel   then per level (FRCNN_CONV_PLAN_MAX_LEVELS x 4; zeros past n_levels)
 *            [0] segments per tile row   [1] tile rows per strip   [2] tile rows of the last strip where it is partial, else 0   [3] tiles of the last segment
 *            where it is partial, else 0
 * Returns FRCNN_OK, or FRCNN_ERR_UNSUPPORTED / FRCNN_ERR_INVALID_ARG where the forward would not take the shapes. */
#define FRCNN_CONV_SCHED_STREAM_K 0        /* ranges of K chunks across tile boundaries: partial tiles, slabs, tickets */
#define FRCNN_CONV_SCHED_WHOLE_RANGES 1    /* several tiles per workgroup, ranges cut at tile boundaries */
#define FRCNN_CONV_SCHED_ONE_TILE 2        /* one whole tile per workgroup, G = n_tiles */
#define FRCNN_CONV_SCHED_FUSED_OUT64 3     /* 64 -> 64 on the 4 x 4 tile: product and output transform in one kernel (no product tiles: [6]..[8] are what the unfused product would have) */
#define FRCNN_CONV_PLAN_MAX_LEVELS 8
#define FRCNN_CONV_PLAN_HEAD 8
#define FRCNN_CONV_PLAN_PRODUCT 10
#define FRCNN_CONV_PLAN_STRIPS (2 + 4 * FRCNN_CONV_PLAN_MAX_LEVELS)
#define FRCNN_CONV_PLAN_INTS (FRCNN_CONV_PLAN_HEAD + 3 * FRCNN_CONV_PLAN_PRODUCT + 2 * FRCNN_CONV_PLAN_STRIPS)
int frcnn_conv3x3_f32_plan(const int *H_host, const int *W_host, int n_levels, int Cin, int Cout, int *plan_host, int plan_len);
/* How the stage's products (M = U . V per Winograd plane; the weight gradient's dU = dM . V^T) are taken -- a process-wide switch, 0 by default:
 *   0  v_mfma_f32_32x32x2_f32 on the fp32 operands;
 *   1  the same fp32 operands cut into three bf16 pieces each in registers (exactly) and six v_mfma_f32_32x32x16_bf16 per 16 k rows, fp32 accumulation:
 *      against float64 as close as mode 0 (tests/test_gpu_ops.py: test_conv3x3_f32_split_products_*), 1.4-1.5 x the rate.  Inputs, outputs, workspaces and
 *      every other kernel of the stage are the same.  Environment: FRCNN_CONV_F32_PRODUCTS=split sets the initial value.
 * The switch also governs frcnn_gemm_nt_f32 (the 1 x 1 weight gradients: the same product kernel).  It does not reach the fused 64 -> 64 product on
 * 4 x 4 tiles (rpn_wino_gemm_out64_kernel), which stays on the fp32 instruction in either mode.  Mode 1's cut is exact for |v| >= 2^-110 and 0; below,
 * the smallest piece falls under fp32's normal range and is lost (error < 2^-126 per operand; tests/test_gpu_products_numerics.py).
 * Returns the previous mode; mode < 0 only asks. */
int frcnn_conv3x3_f32_products(int mode);
int frcnn_conv3x3_f32_fwd(const float *const *x_levels, float *const *y_levels, const int *H_host, const int *W_host, int n_levels, int Cin, int Cout,
                          const float *w, const float *bias, int relu, unsigned short *relu_bits, float *x_transformed, float *u_rotated, void *workspace,
                          size_t workspace_bytes, void *stream);
int frcnn_conv3x3_f32_bwd_data(const float *const *dy_levels, const unsigned short *relu_bits, float *const *dx_levels, const int *H_host, const int *W_host,
                               int n_levels, int Cin, int Cout, const float *w, const float *u_rotated, int pooled, float *dy_transformed,
                               int want_bias_partials, void *workspace, size_t workspace_bytes, void *stream);
int frcnn_conv3x3_f32_wgrad(const float *const *x_levels, const float *const *dy_levels, const unsigned short *relu_bits, const int *H_host, const int *W_host,
                            int n_levels, int Cin, int Cout, float *dw, float *dbias, const float *x_transformed, int pooled, const float *dy_transformed,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Both gradients of a layer whose forward kept x_transformed, in ONE call: bit for bit what _bwd_data (given dy_transformed, want_bias_partials = dbias != NULL)
 * followed by _wgrad (given x_transformed and that dy_transformed) leave in dx_levels, dy_transformed, dw and dbias, in fewer launches -- the data gradient's
 * output transform and the weight gradient's last kernel, which do not depend on each other, share one, and so do the two products on the tile shapes where
 * that was measured to gain (given u_rotated; each product keeps its ranges and its order of summation).  x_transformed, dy_transformed (scratch of
 * frcnn_conv3x3_f32_xt_floats(H, W, n_levels, Cout) floats) and dw are required; relu_bits, u_rotated and dbias are optional as in the two calls; Cin and
 * Cout multiples of 64.  A caller that wants one gradient only, or has no cached transform, makes the two calls above. */
int frcnn_conv3x3_f32_bwd(const float *const *dy_levels, const unsigned short *relu_bits, float *const *dx_levels, const int *H_host, const int *W_host,
                          int n_levels, int Cin, int Cout, const float *w, const float *u_rotated, int pooled, const float *x_transformed,
                          float *dy_transformed, float *dw, float *dbias, void *workspace, size_t workspace_bytes, void *stream);

/* O[m][n] = sum_k A[m][k] * B[n][k], fp32, both operands with k contiguous (the conv stage's weight-gradient GEMM on its own; fixed summation order).  The
 * weight gradient of a 1 x 1 convolution is this product on the NCHW planes as they are: dW [Cout, Cin] = dY [Cout, H*W] . X [Cin, H*W]^T -- the bottlenecks'
 * and the FPN laterals' 1 x 1 convolutions behind models/new_model.py:372.  M, N multiples of 64 (<= 4096); splits >= 1 cuts K into equal pieces with
 * one partial product each, O [splits, M, N] (the caller adds them in order; keeps a long K from being one tile's many slabs); K a multiple of 32 * splits.  workspace: the conv
 * stage's dedicated zero-before-first-use block (>= frcnn_gemm_nt_f32_workspace() bytes; any block sized by frcnn_conv3x3_f32_workspace is larger). */
size_t frcnn_gemm_nt_f32_workspace(void);
int frcnn_gemm_nt_f32(const float *A, const float *B, float *O, int M, int N, int K, int splits, void *workspace, size_t workspace_bytes, void *stream);

/* The backbone's FIRST convolution, nn.Conv2d(3, Cout, 3, padding=1) (+ ReLU): `vgg16.features[0]` + `[1]` behind models/model.py:279-281.  Three input
 * channels are no contraction for the matrix cores: a byte mover on the vector units (csrc/conv_c3.hip).  x [3, H, W], y / dy [Cout, H, W], w [Cout, 3, 3, 3],
 * fp32, batch 1.  relu_bits (optional, ceil(Cout / 64) * H * W uint64 words): the signs of the ReLU outputs, bit co % 64 of word [co / 64][pixel]; _wgrad
 * given the same words counts dy where the bit is set (NULL: dy as it is).  dw [Cout, 3, 3, 3] and dbias [Cout] (or NULL) are fully overwritten; Cout a
 * multiple of 4 and W <= 1700 for _wgrad; workspace >= frcnn_conv3x3_c3_wgrad_workspace(H, Cout) bytes of plain scratch.  No input gradient (the
 * input is the image).  Bit-reproducible. */
int frcnn_conv3x3_c3_fwd(const float *x, float *y, int H, int W, int Cout, const float *w, const float *bias, int relu, unsigned long long *relu_bits,
                         void *stream);
size_t frcnn_conv3x3_c3_wgrad_workspace(int H, int Cout);
int frcnn_conv3x3_c3_wgrad(const float *x, const float *dy, int H, int W, int Cout, const unsigned long long *relu_bits, float *dw, float *dbias,
                           void *workspace, size_t workspace_bytes, void *stream);

/* FrozenBatchNorm2d (+ residual add) (+ ReLU) of torchvision's ResNet bottleneck behind models/new_model.py:372, one pass each way (csrc/affine.hip):
 *   _fwd : y = act((x * scale[c] + shift[c]) [+ res]), the torch form's operations in its order (bit-identical); res may be NULL; act = ReLU when relu != 0.
 *   _bwd : gm = 0 where y <= 0, else g -- also at a NaN y, as torch's threshold_backward -- (relu != 0; y = the forward's output) or g;  dx = gm * scale[c];
 *          dres = gm (NULL: not wanted).
 * x, y, res, g, dx, dres: [C, HW] fp32 (NCHW, batch 1); scale, shift: [C] (the frozen statistics folded as torchvision does). */
int frcnn_affine_act_fwd(const float *x, const float *res, float *y, const float *scale, const float *shift, int C, int HW, int relu, void *stream);
int frcnn_affine_act_bwd(const float *g, const float *y, const float *scale, float *dx, float *dres, int C, int HW, int relu, void *stream);
/* The same passes with bf16 on either side of the fp32 arithmetic (BASELINE configs[4]: bf16 autocast of the backbone; the reference has no mixed-precision
 * mode, torch.autocast over models/new_model.py:372 is what this replaces).  dtype codes: 0 = fp32, 1 = bf16.
 *   _fwd_mixed : x (x_dtype) -> y (y_dtype) = act((x * scale + shift) [+ res fp32]), one rounding on the way out; twin_bf16 (or NULL) receives the same values
 *                rounded to bf16 in the same pass (the next convolutions' input).  Forms: bf16 -> bf16 (no res, no twin); bf16 | fp32 -> fp32 (any).
 *   _bwd_mixed : g, y in y's dtype; g2_bf16 = the gradient that arrived at the twin (or NULL), added to g first; dx in x's dtype; dres fp32 or NULL. */
int frcnn_affine_act_fwd_mixed(const void *x, int x_dtype, const float *res, void *y, int y_dtype, void *twin_bf16, const float *scale, const float *shift,
                               int C, int HW, int relu, void *stream);
int frcnn_affine_act_bwd_mixed(const void *g, int g_dtype, const void *g2_bf16, const void *y, const float *scale, void *dx, int dx_dtype, float *dres,
                               int C, int HW, int relu, void *stream);

/* ---- target makers ------------------------------------------------------------------------------ */
/* RPNTargetMaker.forward: variant 0 = VGG (models/model_.py:186-266), 1 = FPN (models/new_model.py:299-349).
 * Sampling (torch.randperm on the host in the reference, model_.py:228,235):
 *   perm_pos / perm_neg != NULL : consume the reference's permutations (parity mode); their lengths must
 *        equal the positive / negative counts (learn them with a first call and out_counts);
 *   else                        : device Philox4x32-10 keyed by (seed, offset): keep the candidates with the
 *        smallest (key, index).  (seed, offset) come BY VALUE, or -- philox_state_dev != NULL -- from device memory:
 *        philox_state_dev[0] = seed, [1] = offset; the call uses that pair and leaves offset + 1 behind (ABI v4).  A training
 *        step captured in a HIP graph therefore draws fresh samples at every replay; by-value arguments would be frozen in it.
 * out_counts (int32[4], device): {n_pos, n_neg before sampling, error flag, reserved}.
 * workspace: DEDICATED to this entry point and ZERO before the first call.  In device-RNG mode column maxima, labels and (N <= 24 576)
 * sampling run as ONE launch whose workgroups meet at an in-kernel barrier; its arrival counter, last-workgroup ticket and the
 * per-GT maxima live in the workspace and are left zero by every call (no memset node; HIP-graph replays need no clearing).  So are
 * the sampler's key histogram and list counters, which the staged device-RNG form (grids too large to be co-resident) shares.         */
int frcnn_rpn_targets(int variant, const float *anchors /*[N,4]*/, int64_t N, const float *gt /*[G,4]*/, int64_t G,
                      const int64_t *perm_pos, int64_t n_perm_pos, const int64_t *perm_neg, int64_t n_perm_neg,
                      uint64_t seed, uint64_t offset, uint64_t *philox_state_dev /*[2] device, or NULL*/,
                      int64_t *out_cls /*[N]*/, float *out_reg /*[N,4]*/, int32_t *out_counts /*[4]*/,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same with the number of ground-truth boxes as DATA: gt is [G_cap, 4] and *n_gt_dev (device int32, read by every kernel of the call,
 * no host sync) says how many of its rows are live, so a step captured in a HIP graph serves frames with any number of boxes.
 *   n_gt_dev == NULL : all G_cap rows are live -- frcnn_rpn_targets, which is this call with NULL.
 *   otherwise        : G = min(*n_gt_dev, G_cap); outputs, counts and the Philox state are bit for bit those of frcnn_rpn_targets on
 *                      gt[:G].  Rows >= G are never read into a result (they may hold NaN, infinities, copies of anchors).
 * Everything the host decides goes by G_cap: 1 <= G_cap <= 4096, workspace >= frcnn_workspace_bytes(FRCNN_OP_RPN_TARGETS, N, G_cap).
 * The reference raises for a frame without boxes; a captured step cannot, so the two cases outside [1, G_cap] are defined here:
 *   *n_gt_dev > G_cap : the first G_cap rows are used and out_counts[2] carries FRCNN_RPN_ERR_GT_COUNT;
 *   *n_gt_dev <= 0    : every out_cls = -1 (no anchor takes part in the loss), out_reg = 0, out_counts = {0, 0, FRCNN_RPN_ERR_GT_COUNT, 0}.
 * out_counts[2] values: 1 / 2 a permutation's length / an entry is wrong (parity mode), 4 the in-kernel barrier timed out, 8 the
 * sampler's boundary list overflowed; FRCNN_RPN_ERR_GT_COUNT is OR-ed to 1, 2 and 8 (a barrier time-out reports 4 alone).
 * The workspace invariant (left zero by every call) holds for every count, 0 included. */
#define FRCNN_RPN_ERR_GT_COUNT 16       /* *n_gt_dev outside [1, G_cap] */
int frcnn_rpn_targets_n(int variant, const float *anchors /*[N,4]*/, int64_t N, const float *gt /*[G_cap,4]*/, int64_t G_cap,
                        const int32_t *n_gt_dev /* device int32, or NULL */,
                        const int64_t *perm_pos, int64_t n_perm_pos, const int64_t *perm_neg, int64_t n_perm_neg,
                        uint64_t seed, uint64_t offset, uint64_t *philox_state_dev /*[2] device, or NULL*/,
                        int64_t *out_cls /*[N]*/, float *out_reg /*[N,4]*/, int32_t *out_counts /*[4]*/,
                        void *workspace, size_t workspace_bytes, void *stream);

/* FastRcnnTargetMaker.forward (models/model_.py:127-179; FPN: models/new_model.py:157-206).
 * rois [P_cap,4] with a device count n_rois_dev (NULL = P_cap rows are live); candidates = cat(rois, gt).
 * variant 0: find_jaccard_overlap(roi, gt) eps 1e-5; 1: box_iou(gt, roi).  label_offset 1 (VGG) / 0 (FPN);
 * max_pos 32 / 128; total 128 / 512.  out_counts = {#pos cand, #neg cand, rows written, error bits}.
 * Failure is never silent and never needs a host sync: rows beyond the number actually sampled (the reference throws
 * there, model.py:340 / new_model.py:182) get the out-of-range class -1 and zero boxes, and a NEGATIVE *n_rois_dev (the
 * proposal stage reporting an aborted NMS scan) marks every row that way; frcnn_detection_loss turns an out-of-range
 * class into a NaN loss.  The error bits are also OR-ed into *sticky_status (device int32, may be NULL), which the
 * caller reads whenever it syncs anyway (logging / checkpoint interval). */
#define FRCNN_HT_ERR_PERM_LENGTH 1      /* perm_pos / perm_neg length != candidate count (parity mode) */
#define FRCNN_HT_ERR_PERM_RANGE 2       /* a permutation entry is out of range */
#define FRCNN_HT_ERR_UPSTREAM_ABORT 4   /* *n_rois_dev < 0 */
#define FRCNN_HT_ERR_SHORT 8            /* fewer than `total` rows could be sampled */
int frcnn_head_targets(int variant, const float *rois, const int32_t *n_rois_dev, int64_t P_cap,
                       const float *gt, const int64_t *gt_label, int64_t G,
                       int64_t label_offset, int64_t max_pos, int64_t total,
                       const int64_t *perm_pos, int64_t n_perm_pos, const int64_t *perm_neg, int64_t n_perm_neg,
                       uint64_t seed, uint64_t offset, uint64_t *philox_state_dev /*[2] device (see frcnn_rpn_targets), or NULL*/,
                       int64_t *out_cls /*[total]*/, float *out_reg /*[total,4]*/, float *out_rois /*[total,4]*/,
                       int64_t *out_keep_index /*[total] or NULL*/, int32_t *out_counts /*[4]*/,
                       int32_t *sticky_status /* device int32 or NULL */, void *stream);
/* The same with a device count for gt / gt_label ([G_cap, 4] / [G_cap]) as well: see frcnn_rpn_targets_n.  n_gt_dev == NULL is
 * frcnn_head_targets; otherwise the result is bit for bit that of frcnn_head_targets on gt[:G], gt_label[:G], G = min(*n_gt_dev, G_cap).
 * Limits go by G_cap (G_cap >= 1, P_cap + G_cap <= 4096).
 *   *n_gt_dev > G_cap : the first G_cap rows, and FRCNN_HT_ERR_GT_COUNT in out_counts[3] / *sticky_status;
 *   *n_gt_dev <= 0    : every row gets class -1 and zero boxes, as FRCNN_HT_ERR_SHORT rows do; FRCNN_HT_ERR_SHORT | FRCNN_HT_ERR_GT_COUNT.
 * empty_dev (device int32 or NULL) is written by EVERY call: 1 when the frame has no live box, else 0 (not sticky).  It is made to be
 * DeviceSGD's guard word: an empty frame then makes the captured optimizer step a no-op and the next frame trains normally. */
#define FRCNN_HT_ERR_GT_COUNT 16        /* *n_gt_dev outside [1, G_cap] */
int frcnn_head_targets_n(int variant, const float *rois, const int32_t *n_rois_dev, int64_t P_cap,
                         const float *gt /*[G_cap,4]*/, const int64_t *gt_label /*[G_cap]*/, int64_t G_cap,
                         const int32_t *n_gt_dev /* device int32, or NULL */,
                         int64_t label_offset, int64_t max_pos, int64_t total,
                         const int64_t *perm_pos, int64_t n_perm_pos, const int64_t *perm_neg, int64_t n_perm_neg,
                         uint64_t seed, uint64_t offset, uint64_t *philox_state_dev,
                         int64_t *out_cls /*[total]*/, float *out_reg /*[total,4]*/, float *out_rois /*[total,4]*/,
                         int64_t *out_keep_index /*[total] or NULL*/, int32_t *out_counts /*[4]*/,
                         int32_t *sticky_status /* device int32 or NULL */, int32_t *empty_dev /* device int32 or NULL */, void *stream);

/* ---- RoI pooling ---------------------------------------------------------------------------------- */
/* torchvision.ops.RoIPool((PH,PW), spatial_scale) forward/backward (models/model.py:97,113); one image,
 * feat [C,H,W] fp32 NCHW, rois [R,4] = x1,y1,x2,y2 (the reference pre-multiplies by (fw,fh)). */
int frcnn_roi_pool_fwd(const float *feat, int C, int H, int W, const float *rois, int64_t R, int PH, int PW,
                       float spatial_scale, float *out /*[R,C,PH,PW]*/, int32_t *argmax /*[R,C,PH,PW]*/, void *stream);
/* grad_feat [C,H,W] is fully overwritten (no pre-zeroing needed). */
int frcnn_roi_pool_bwd(const float *grad_out, const int32_t *argmax, int64_t R, int C, int H, int W, int PH, int PW,
                       float *grad_feat, void *stream);
/* The same 7x7 pooling with a library-private 16-bit argmax (0xFFFF = empty bin) for planes of fewer than 65535 pixels that
 * fit the LDS-staged kernel (4*H*W*4 bytes <= 48 KB): what the host layer's autograd pair uses (models/model.py:113 never sees
 * the argmax).  Same `out` / `grad_feat` as the int32 entry points; 2 bytes less per pooled element to write and to read back. */
int frcnn_roi_pool_fwd_a16(const float *feat, int C, int H, int W, const float *rois, int64_t R, float spatial_scale,
                           float *out /*[R,C,7,7]*/, uint16_t *argmax16 /*[R,C,7,7]*/, void *stream);
/* `rois` / `spatial_scale`: the boxes the forward pooled (may be NULL).  With them the backward adds without LDS atomics for every RoI of at
 * least 7 x 7 feature cells; without them, and for smaller RoIs, with ds_add_f32.  For an even C the result is bit-reproducible run to run;
 * an odd C takes the shared-plane kernel, whose LDS atomics add in arrival order (last-bit differences between runs). */
int frcnn_roi_pool_bwd_a16(const float *grad_out, const uint16_t *argmax16, const float *rois /*[R,4] or NULL*/, float spatial_scale,
                           int64_t R, int C, int H, int W, float *grad_feat, void *stream);
/* What the four entry points above execute for a shape: the host functions the launches use; no device is touched, nothing is launched.
 * argmax16: the 16-bit pair (PH = PW = 7) instead of the int32 pair; have_rois: frcnn_roi_pool_bwd_a16 is given the boxes.  R >= 1.
 * plan_host receives FRCNN_ROI_PLAN_INTS ints (plan_len >= that):
 *   [0] forward form (FRCNN_ROI_FWD_*; -1: the entry point refuses the shape)   [1] S = RoI slices (grid.y)   [2] RB = RoIs per workgroup
 *   [3] 1 when the launch asks for 84 KB of LDS to have a CU to itself   [4] the forward's dynamic LDS bytes  ([1]..[4] are 0 for the generic form)
 *   [5] backward form (FRCNN_ROI_BWD_*; -1: refused)   [6] the backward's dynamic LDS bytes
 *   [7] 1 when RoIs of at least 7 x 7 cells add in rank order without LDS atomics (a wave-private form that is given the boxes)
 * The environment variable FRCNN_ROI_BWD_SHARED (any value) makes the 16-bit backward take the shared-plane form, here as in the launch. */
#define FRCNN_ROI_FWD_LDS 0                /* planes staged in LDS, dynamic task queue: 7 x 7 bins, 16 * H * W <= 48 KB */
#define FRCNN_ROI_FWD_GENERIC 1            /* one lane per output element */
#define FRCNN_ROI_BWD_PRIVATE8 0           /* wave-private planes, 8 copies: 16-bit argmax, even C */
#define FRCNN_ROI_BWD_PRIVATE4 1           /* ... 4 copies */
#define FRCNN_ROI_BWD_SHARED_CB 2           /* two channels per workgroup, one plane each, LDS atomics */
#define FRCNN_ROI_BWD_ONE_CHANNEL 3        /* one channel per workgroup, any bin grid */
#define FRCNN_ROI_BWD_GLOBAL_ATOMIC 4      /* memset + global fp32 atomics */
#define FRCNN_ROI_PLAN_INTS 8
int frcnn_roi_pool_plan(int C, int H, int W, int64_t R, int PH, int PW, int argmax16, int have_rois, int *plan_host, int plan_len);

/* torchvision.ops.MultiScaleRoIAlign(names, PH, sampling_ratio) (models/new_model.py:127,143): level mapper
 * k = floor(k0 + log2(sqrt(area)/s0) + 1e-6) clamped to [k_min, k_min+n_levels-1]; per level roi_align
 * (aligned = False).  rois in image pixels.  The per-level scales are explicit.            */
int frcnn_roi_level_map(const float *rois, int64_t R, int k_min, int k_max, float s0, int k0, float eps,
                        int32_t *out_level, void *stream);
int frcnn_ms_roi_align_fwd(const float *const *feats_host /*[n_levels] device ptrs*/, const int *H_host, const int *W_host,
                           const float *scales_host, int n_levels, int C, const float *rois, int64_t R,
                           int PH, int PW, int sampling_ratio, int aligned, int k_min, float s0, int k0,
                           float *out /*[R,C,PH,PW]*/, int32_t *out_level /*[R] or NULL*/,
                           const int32_t *order /*[R] or NULL: dispatch order of the RoIs (frcnn_roi_scale_order); results do not depend on it*/,
                           void *stream);
/* The `roi * (w, h, w, h)` of FastRCNNHead.forward (models/new_model.py:136-140) and, in the same launch, the permutation that
 * dispatches the 7x7 / sampling-ratio-2 forward's workgroups largest footprint first: out_rois[i] = rois[i] * mul4 (fp32 products, as
 * torch computes them), out_order = RoI indices by decreasing (staging passes, footprint pixels) of frcnn_ms_roi_align_fwd, ties by
 * index; out_cost (optional, [R]) = the keys.  R <= 4096.  Level table as in frcnn_ms_roi_align_fwd (no feature pointers needed).  */
int frcnn_roi_scale_order(const float *rois, int64_t R, const float *mul4_host, const int *H_host, const int *W_host, const float *scales_host,
                          int n_levels, int aligned, int k_min, float s0, int k0, float *out_rois /*[R,4] or NULL*/, int32_t *out_order /*[R]*/,
                          uint32_t *out_cost /*[R] or NULL*/, void *stream);
/* grad_feats[l] [C,H_l,W_l] are OVERWRITTEN with the gradient of every level (zero where no RoI reaches); the caller does
 * not clear them.  7x7 / sampling_ratio 2: tile-owner gather (per-tile RoI lists, long lists summed by segments in a fixed
 * order), no atomics, bit-reproducible, two launches; workspace >= frcnn_ms_roi_align_bwd_workspace(...) (lists, weight-table
 * records of the (RoI, tile) pairs, partial tiles, tickets; its contents on entry do not matter).  One call at a time per
 * device (the last-workgroup ticket of the lists launch is a word of the library picked by the workspace address).  Other
 * shapes: memset + fp32 atomics inside the library (sum order not fixed, tolerance 1e-4; no workspace needed).             */
size_t frcnn_ms_roi_align_bwd_workspace(const int *H_host, const int *W_host, int n_levels, int C, int64_t R);
int frcnn_ms_roi_align_bwd(const float *grad_out, float *const *grad_feats_host, const int *H_host, const int *W_host,
                           const float *scales_host, int n_levels, int C, const float *rois, int64_t R,
                           int PH, int PW, int sampling_ratio, int aligned, int k_min, float s0, int k0,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- detection losses (losses/loss.py:5-85) ------------------------------------------------- */
/* FRCNNLoss forward AND the un-normalised input gradients in one pass.  out7 (device): total, rpn_cls, rpn_reg,
 * head_cls, head_reg losses, then 1/#(rpn label >= 0) and 1/R (the scales backward multiplies the gradients by).
 * g_* have the shapes of the predictions; every row is written (zeros for an ignored row), so their contents on entry
 * do not matter.
 * Labels that are no class: a head class outside [0, NC) (compared in 64 bits, so 2^32 + 3 is no class 3) and an RPN
 * label above 1 are both the failure mark.  That part's CE term and the total become NaN (the reference's cross_entropy
 * throws there); the row's class gradient is the plain softmax (finite, no one-hot subtracted); the row counts in
 * #(rpn label >= 0), and its regression terms count as for any other label > 0 (the 64-bit label decides).
 * workspace >= 32 KiB, DEDICATED to this entry point and ZERO before the first call: its first word is the ticket
 * by which the last workgroup to finish adds up the partial sums (one launch, no finalize kernel); that workgroup leaves the ticket zero, so consecutive calls (and HIP-graph replays) need no clearing in between.            */
int frcnn_detection_loss(const float *rpn_cls /*[N,2]*/, const float *rpn_reg /*[N,4]*/, const int64_t *t_rpn_cls /*[N]*/,
                         const float *t_rpn_reg /*[N,4]*/, int64_t N,
                         const float *head_cls /*[R,NC]*/, const float *head_reg /*[R,4]*/, const int64_t *t_cls /*[R]*/,
                         const float *t_reg /*[R,4]*/, int64_t R, int NC,
                         float *out7, float *g_rpn_cls, float *g_rpn_reg, float *g_head_cls, float *g_head_reg,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- detection post-process (models/model.py:368-402, models/new_model.py:420-470) ------------------------------ */
/* The post-processing half of FRCNN.predict in three launches and no host sync (graph-capturable): for every live row
 * r < *n_rois_dev, prob[r] = softmax(head_cls[r]) (fp32) and, for every class c in 1 .. C-1,
 *   box = clamp01(cxcy_to_xy(decode(head_reg[r,c] * (0.1, 0.1, 0.2, 0.2), xy_to_cxcy(rois[r]))))   (bit-identical to frcnn_box_codec);
 * then _suppress: per class the candidates prob[r,c] > thr (strict, fp32; thr = *threshold_dev when given, else threshold),
 * greedy NMS in descending score (ties: ascending r) with frcnn_nms_classed's IoU decision (> nms_threshold, strict), and the
 * CLASS-MAJOR concatenation: class 1 first, score order inside a class, labels c - 1.  *out_count = the total (<= (C-1)*P);
 * out_class_counts[c-1] (optional) the per-class counts.  Rows >= *n_rois_dev are never detections (they may hold NaN).
 * *n_rois_dev < 0 (an aborted proposal scan upstream) gives *out_count = -1.  out_prob (optional) receives the softmax.
 * Limits: 1 <= P <= 2048, 2 <= C <= 256 (FRCNN_ERR_UNSUPPORTED otherwise).  out_boxes 16-byte aligned.
 * workspace: frcnn_workspace_bytes(FRCNN_OP_DETECT, P, C) bytes, any content.                                        */
int frcnn_detect_postprocess(const float *head_cls /*[P,C] logits*/, const float *head_reg /*[P,4C] raw deltas*/,
                             const float *rois /*[P,4] normalised xyxy*/, const int32_t *n_rois_dev /*live rows, <= P*/,
                             int64_t P, int C, float threshold, const float *threshold_dev /*device float or NULL*/,
                             float nms_threshold,
                             float *out_boxes /*[(C-1)*P,4]*/, int32_t *out_labels /*[(C-1)*P]*/, float *out_scores /*[(C-1)*P]*/,
                             int32_t *out_count /*[1]*/, int32_t *out_class_counts /*[C-1] or NULL*/,
                             float *out_prob /*[P,C] or NULL*/,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- merge of detection sets (test-time augmentation; defined by this project, docs/PARITY.md) --------------------- */
/* Bits of *out_status (0 = nothing to report).  ABORT, CLASS_OVERFLOW and OUTPUT_OVERFLOW also give *out_count = -1. */
#define FRCNN_MERGE_COUNT_CLIPPED 1u     /* a set's count exceeded its capacity: the capacity was used */
#define FRCNN_MERGE_UPSTREAM_ABORT 2u    /* a set's count was negative (an aborted scan upstream): the set contributes nothing */
#define FRCNN_MERGE_LABEL_RANGE 4u       /* a live row's label lay outside 0 .. C-2: the row was skipped */
#define FRCNN_MERGE_CLASS_OVERFLOW 8u    /* a class held more than FRCNN_MERGE_MAX_CANDIDATES candidates: the class comes out empty */
#define FRCNN_MERGE_OUTPUT_OVERFLOW 16u  /* the kept total exceeded out_capacity: the rows past it were not written */
#define FRCNN_MERGE_MAX_SETS 8
#define FRCNN_MERGE_MAX_CANDIDATES 2048
/* K fixed-capacity detection sets with device counts -> one set of the same shape, in two launches whatever the data holds and no host
 * sync (graph-capturable).  The six per-set arrays are HOST arrays of K entries; their values travel by value in the kernel arguments,
 * so nothing host-side is read when a captured graph replays.  Everything below is device data.
 * Transform: set k's live rows are 0 .. *counts[k]-1; a count above caps[k] uses caps[k] (COUNT_CLIPPED); a negative count makes the set
 *   contribute nothing and gives *out_count = -1 (UPSTREAM_ABORT).  flags[k] bit 0: the view was mirrored horizontally, the box becomes
 *   (1.0f - x2, y1, 1.0f - x1, y2), one fp32 subtraction each; bit 1: the same for y.  No other transform.  Areas are
 *   (x2 - x1) * (y2 - y1) in fp32 on the transformed box.
 * Candidates: one workgroup per class c in 0 .. C-2 (labels are 0-based) takes every live row of every set with label c and
 *   score > min_score (strict: NaN, and with min_score = 0 non-positive scores, drop out), whatever the order of the rows.  A live row
 *   whose label lies outside 0 .. C-2 is skipped, whatever its score (LABEL_RANGE).  More than 2048 candidates in a class: the class
 *   comes out empty and *out_count = -1 (CLASS_OVERFLOW).
 * Order: score descending (-0 counts as +0), then set index ascending, then row ascending.
 * Suppression: greedy in that order with frcnn_nms_classed's IoU decision (> nms_threshold, strict; a NaN or zero-area box is never
 *   suppressed and suppresses nothing).  With K = 1, no flip and voting off, a set that left frcnn_detect_postprocess with the same
 *   nms_threshold comes back bit for bit.
 * Box voting (vote_threshold >= 0; < 0 or NaN = off), Detectron's box_voting in its ID scoring mode: the voters of kept box i are i
 *   itself, always, and every candidate j of the class, suppressed or not, with IoU(i, j) >= vote_threshold -- the quotient of the
 *   suppression's fp32 expression.  Scores, labels and order are unchanged; coordinate x of box i becomes
 *   float32(sum_j s_j x_j / sum_j s_j), the five sums in binary64 in this order: lane l of the box's wave adds the voters at sorted
 *   positions p = l (mod 64) in ascending p onto +0.0, each term the exact product (double)s_j * (double)x_j (for the weight sum,
 *   (double)s_j); the 64 partials are combined by an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (every lane adds its partner's value to its
 *   own); then one binary64 division and one rounding to fp32.  The box keeps its original bits when i is its only voter, when any of the
 *   five sums is not finite, or when the weight sum is not > 0.  For vote_threshold > 0 a NaN or zero-area box is its own only voter.
 * Emit: class-major concatenation, suppression order inside a class; *out_count = the kept total, out_class_counts[c] (optional) the
 *   per-class counts, *out_status (optional) the bits above.  A kept total above out_capacity gives *out_count = -1 (OUTPUT_OVERFLOW);
 *   nothing is written past out_capacity.  Rows at and above the count are left as they were.
 * Limits: 1 <= K <= 8, 0 <= caps[k] <= 2^28, 2 <= C <= 256 (FRCNN_ERR_UNSUPPORTED otherwise for C and caps above 2^28;
 * FRCNN_ERR_INVALID_ARG for NULL pointers, K, negative capacities, boxes or out_boxes not 16-byte aligned).
 * workspace: frcnn_workspace_bytes(FRCNN_OP_DETECT_MERGE, out_capacity, C) bytes, any content. */
int frcnn_detect_merge(int K, const float *const *boxes /*[caps[k],4] xyxy*/, const int32_t *const *labels /*[caps[k]]*/,
                       const float *const *scores /*[caps[k]]*/, const int32_t *const *counts /*[1]*/, const int64_t *caps,
                       const uint32_t *flags, int C, float min_score, float nms_threshold, float vote_threshold,
                       float *out_boxes /*[out_capacity,4]*/, int32_t *out_labels /*[out_capacity]*/, float *out_scores /*[out_capacity]*/,
                       int32_t *out_count /*[1]*/, int32_t *out_class_counts /*[C-1] or NULL*/, int32_t *out_status /*[1] or NULL*/,
                       int64_t out_capacity, void *workspace, size_t workspace_bytes, void *stream);

/* Soft-NMS (Bodla et al., 2017) as the merge's suppression step: defined by this project, restated from the published algorithm. */
#define FRCNN_SOFT_NMS_HARD 0       /* an overlapped candidate is dropped: frcnn_detect_merge's result, bit for bit */
#define FRCNN_SOFT_NMS_LINEAR 1     /* its score is multiplied by 1 - IoU */
#define FRCNN_SOFT_NMS_GAUSSIAN 2   /* its score is multiplied by exp(-IoU^2 / sigma) */
/* frcnn_detect_merge with another suppression step.  Transform, Candidates, Order, Box voting, Emit, Limits, the workspace
 * (FRCNN_OP_DETECT_MERGE), the status bits, the -1 counts and the refusals are frcnn_detect_merge's, word for word; two launches whatever
 * the data holds, graph-capturable, the per-set rows by value in the kernel arguments.  The order gives every candidate of a class a sorted
 * position p.
 * Suppression: every candidate p carries a working score w_p (fp32), at first its own score.  While a candidate is live:
 *   1. Pick the live candidate with the largest w, on a tie the smallest p (-0 counts as +0: the order of the candidates' keys).
 *   2. Emit it with score w and its (flipped-back) box; it is no longer live.  Scores are therefore non-increasing inside a class.
 *   3. For every live j: ov = the fp32 IoU quotient of the suppression decision (picked box, box j); a NaN ov decays nothing.
 *        HARD:     ov > nms_threshold (strict): j is dropped.
 *        LINEAR:   ov > nms_threshold: w_j = w_j * (1.0f - ov), one fp32 subtraction and one fp32 multiplication.
 *        GAUSSIAN: ov > 0: w_j = w_j * (float)exp(-((double)ov * (double)ov) / (double)sigma): the weight in binary64 (the device's exp,
 *                  within an ulp of it), rounded once to fp32, then one fp32 multiplication.  nms_threshold is not read.
 *      After a decay j stays live only if w_j >= score_floor (a NaN drops).  A candidate that was never decayed is never tested against
 *      the floor.  For nms_threshold >= 0 a NaN or zero-area box is never decayed, decays nobody and is emitted at its own score: its
 *      ov is NaN or 0.
 * Box voting: as frcnn_detect_merge -- the voters of an emitted box are itself and every candidate of the class, live, dropped or emitted,
 *   with IoU >= vote_threshold, weighted by their ORIGINAL scores in the binary64 order stated there; the emitted score is the working score.
 * Cost: one step per candidate of a class, the classes in parallel (the greedy scan skips suppressed boxes, this one cannot).
 * FRCNN_ERR_INVALID_ARG also for a method outside 0 .. 2, a sigma that is not > 0 in GAUSSIAN mode, and a NaN score_floor. */
int frcnn_detect_merge_soft(int K, const float *const *boxes /*[caps[k],4] xyxy*/, const int32_t *const *labels /*[caps[k]]*/,
                            const float *const *scores /*[caps[k]]*/, const int32_t *const *counts /*[1]*/, const int64_t *caps,
                            const uint32_t *flags, int C, float min_score, float nms_threshold, float vote_threshold, int method, float sigma,
                            float score_floor, float *out_boxes /*[out_capacity,4]*/, int32_t *out_labels /*[out_capacity]*/,
                            float *out_scores /*[out_capacity]*/, int32_t *out_count /*[1]*/, int32_t *out_class_counts /*[C-1] or NULL*/,
                            int32_t *out_status /*[1] or NULL*/, int64_t out_capacity, void *workspace, size_t workspace_bytes, void *stream);

/* ---- detection evaluator: the VOC AP protocol (evaluation/voc_eval.py:67-112,115-135,138-225) ------------------------ */
/* Flags of a record: 2 bits per threshold t (bits 2t, 2t+1). */
#define FRCNN_EVAL_TP 1u
#define FRCNN_EVAL_FP 2u
#define FRCNN_EVAL_IGNORED 3u      /* the best match is a difficult ground truth at >= t: neither (voc_eval.py:185) */
/* One frame in one launch and no host sync (graph-capturable): replaces save_pred's pixel boxes (voc_eval.py:84-91), save_gt's
 * gt_counter_per_class (:46-56) and cal_mAP's match and decision (:156-197) for the detections of one image.
 *   boxes / labels / scores / count_dev: the tensors of frcnn_detect_postprocess (normalised fp32 xyxy, 0-based labels, *count_dev live
 *   rows of det_capacity); gt_boxes fp32 pixel xyxy, gt_labels in the same label space, gt_difficult 0 / 1, *n_gt_dev live rows of
 *   gt_capacity; frame_dev = (original width, original height, image_id); thresholds_dev = T IoU thresholds (float64).  Everything
 *   that varies per frame is read on the device when the kernel runs.
 * Pixel box = double(box) * double(w or h); the match is the same-class ground truth of the largest float64 overlap with the
 * devkit's +1 convention, first wins ties, used and difficult ones included; at threshold t a detection whose overlap is >= t is
 * IGNORED when the match is difficult, TP when it is the first of the frame's detections (score descending, position ascending) that
 * share the match and reach t, FP otherwise; a detection below t or without a same-class ground truth is FP.
 * Effects: npos[l] += 1 for every non-difficult ground truth; *cursor += count (ONE atomic add; slots past record_capacity are counted,
 * not written); records (score, label, image_id, position, flags) in the reserved slots, in any order -- the defined order of the set
 * is (score descending, image_id ascending, position ascending).  *error_word |= 1 when *count_dev < 0 (an aborted proposal scan
 * upstream), 2 when *n_gt_dev > gt_capacity, 4 when *count_dev > det_capacity, 8 for a label outside 0 .. C-2; a frame with bit 1, 2
 * or 4 is not recorded.
 * Limits (FRCNN_ERR_UNSUPPORTED otherwise): 2 <= C <= 256, 1 <= det_capacity <= (C-1) * 2048, 1 <= gt_capacity <= 1024, 1 <= T <= 16.
 * boxes and gt_boxes 16-byte aligned.  workspace: frcnn_workspace_bytes(FRCNN_OP_EVAL, det_capacity, gt_capacity) bytes, DEDICATED to
 * this entry point and ZERO before the first call (a ticket and the per-ground-truth winner words; the kernel leaves them zero). */
int frcnn_eval_update(const float *boxes /*[D,4]*/, const int32_t *labels /*[D]*/, const float *scores /*[D]*/, const int32_t *count_dev,
                      int64_t det_capacity, const float *gt_boxes /*[G,4] pixels*/, const int32_t *gt_labels /*[G]*/,
                      const uint8_t *gt_difficult /*[G]*/, const int32_t *n_gt_dev, int64_t gt_capacity,
                      const int32_t *frame_dev /*[3]: w, h, image_id*/, const double *thresholds_dev /*[T]*/, int T, int C,
                      int64_t *npos /*[C-1]*/, float *rec_score, int32_t *rec_label, int32_t *rec_image, int32_t *rec_position,
                      uint32_t *rec_flags, int64_t record_capacity, int64_t *cursor /*[1]*/, int32_t *error_word /*[1]*/,
                      void *workspace, size_t workspace_bytes, void *stream);
/* Precision / recall and voc_ap (voc_eval.py:199-219, 115-135) of every class at every threshold, once per test set.  labels_sorted /
 * flags_sorted: the records ordered by (label ascending, score descending, image_id ascending, position ascending), the first
 * min(*n_dev, capacity) rows live.  ap[t, c] (float64) = NaN when npos[c] == 0 (a class the reference does not know), else the sum of
 * (rec[i] - rec[i-1]) * mpre[i] over the points where recall changes, added in ascending order like the reference; tp_total /
 * fp_total [T, C-1] the counts.  Limits: 2 <= C <= 256, 1 <= T <= 16.  workspace >= 256 + 8 * capacity bytes, any content. */
int frcnn_eval_average_precision(const int32_t *labels_sorted, const uint32_t *flags_sorted, const int64_t *n_dev, int64_t capacity,
                                 const int64_t *npos /*[C-1]*/, int T, int C, double *ap /*[T,C-1]*/, int64_t *tp_total /*[T,C-1]*/,
                                 int64_t *fp_total /*[T,C-1]*/, void *workspace, size_t workspace_bytes, void *stream);

/* ---- detection evaluator: the COCO protocol, bbox, useCats = 1 (evaluation/coco_eval.py, test.py:60-88,124-128) --------- */
/* One frame in one launch and no host sync (graph-capturable): replaces CocoEvaluator.update (evaluation/coco_eval.py: prepare_for_coco_detection,
 * convert_to_xywh, COCOeval.evaluate -> computeIoU / evaluateImg) and the pixel boxes of test.py:68-71 for the detections of one image.
 *   boxes / labels / scores / count_dev: the tensors of frcnn_detect_postprocess (normalised fp32 xyxy, 0-based labels, *count_dev live
 *   rows of det_capacity, in ANY order); gt_boxes float64 pixel xywh, gt_area float64 (the annotation's own area), gt_labels in the same
 *   label space, gt_iscrowd 0 / 1, *n_gt_dev live rows of gt_capacity; frame_dev = (original width, original height, image_id);
 *   thresholds_dev = T IoU thresholds (float64).  Everything that varies per frame is read on the device when the kernel runs.
 * Pixel box in fp32: X1 = x1 * w, ..., W = X2 - X1, H = Y2 - Y1, widened to float64; area = W * H.  Per category the detections are
 * ranked by (score descending, position ascending) and cut to max_det (<= 100).  IoU is maskUtils.iou on boxes in float64 (crowd: union
 * = the detection's area).  Area ranges: all, small, medium, large = [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10]; a ground truth
 * is ignored in a range when it is crowd or its area lies outside.  Matching is COCOeval.evaluateImg per (area range, threshold): the
 * non-ignored ground truths first, the ignored ones only when none of the first matched, matched non-crowd ground truths skipped, the
 * later of equal IoUs wins; an unmatched detection whose area lies outside the range is ignored.
 * Effects: npig[l, a] += 1 for every ground truth not ignored in range a; *cursor += the kept detections (one atomic add per category
 * present; slots past record_capacity are counted, not written); records (score, label, image_id, rank in its image and category,
 * flags[4]: per area range 2 bits per threshold, FRCNN_EVAL_TP = matched and not ignored, FRCNN_EVAL_FP = unmatched and not ignored,
 * FRCNN_EVAL_IGNORED otherwise) in the reserved slots, in any order -- the defined order of the set is (label ascending, score
 * descending, image_id ascending, rank ascending).  *error_word |= 1 when *count_dev < 0, 2 when *n_gt_dev > gt_capacity, 4 when
 * *count_dev > det_capacity, 8 for a detection or ground-truth label outside 0 .. C-2; a frame with any of them is not recorded.
 * Limits (FRCNN_ERR_UNSUPPORTED otherwise): 2 <= C <= 256, 1 <= det_capacity <= (C-1) * 2048, 1 <= gt_capacity <= 1024, 1 <= T <= 16,
 * 1 <= max_det <= 100.  boxes 16-byte aligned.  workspace: frcnn_workspace_bytes(FRCNN_OP_COCO_EVAL, det_capacity, gt_capacity) bytes,
 * any content, not shared with a call that may run at the same time. */
int frcnn_coco_eval_update(const float *boxes /*[D,4]*/, const int32_t *labels /*[D]*/, const float *scores /*[D]*/, const int32_t *count_dev,
                           int64_t det_capacity, const double *gt_boxes /*[G,4] pixel xywh*/, const double *gt_area /*[G]*/,
                           const int32_t *gt_labels /*[G]*/, const uint8_t *gt_iscrowd /*[G]*/, const int32_t *n_gt_dev, int64_t gt_capacity,
                           const int32_t *frame_dev /*[3]: w, h, image_id*/, const double *thresholds_dev /*[T]*/, int T, int C, int max_det,
                           int64_t *npig /*[C-1,4]*/, float *rec_score, int32_t *rec_label, int32_t *rec_image, int32_t *rec_rank,
                           uint32_t *rec_flags /*[record_capacity,4]*/, int64_t record_capacity, int64_t *cursor /*[1]*/,
                           int32_t *error_word /*[1]*/, void *workspace, size_t workspace_bytes, void *stream);
/* COCOeval.accumulate (evaluation/coco_eval.py: CocoEvaluator.accumulate, test.py:124-128), once per test set.  labels_sorted /
 * ranks_sorted / flags_sorted [capacity,4]: the records ordered by (label ascending, score descending, image_id ascending, rank
 * ascending), the first min(*n_dev, capacity) rows live.  For every category k, area range a and M in (max_det_0, max_det_1, max_det_2)
 * over the records of rank < M: tp / fp cumulative sums, rc = tp / npig, pr = tp / (fp + tp + 2^-52), pr made non-increasing from the
 * right; recall[t,k,a,m] = rc[-1] (0 without detections); precision[t,r,k,a,m] = pr[searchsorted(rc, rec_thresholds[r], 'left')], 0
 * past the end; both -1 where npig[k,a] == 0.  precision float64 [T,R,C-1,4,3], recall float64 [T,C-1,4,3].
 * Limits: 2 <= C <= 256, 1 <= T <= 16, 1 <= R <= 256.  workspace >= 256 + 32 * capacity bytes, any content. */
int frcnn_coco_eval_accumulate(const int32_t *labels_sorted, const int32_t *ranks_sorted, const uint32_t *flags_sorted, const int64_t *n_dev,
                               int64_t capacity, const int64_t *npig /*[C-1,4]*/, const double *rec_thresholds_dev /*[R]*/, int R, int T, int C,
                               int max_det_0, int max_det_1, int max_det_2, double *precision, double *recall, void *workspace,
                               size_t workspace_bytes, void *stream);
/* The same frame with every category POOLED: COCOeval with useCats = 0 (proposal recall AR@100 / 300 / 1000, class-agnostic AP).  The
 * arguments are those of frcnn_coco_eval_update; two launches whatever the data holds, no host sync (graph-capturable), no workgroup
 * that waits on another.
 *   Pooled lists: the frame's detections and its ground truths are each ONE list in the order (label ascending, original position
 *   ascending) -- pycocotools' [_ for cId in catIds for _ in self._dts[img, cId]].  The detections are ranked by score descending with a
 *   stable sort over that order (equal scores: label ascending, then position ascending) and cut to max_det.  Labels only order the lists
 *   and are range-checked; a detection may match a ground truth of ANY label.
 *   Pixel boxes, the float64 IoU (crowd: union = the detection's area), the area ranges and gtIg = crowd or area outside the range are
 *   those of frcnn_coco_eval_update.  Matching is COCOeval.evaluateImg per (area range, threshold) over the pooled lists: the walk starts
 *   from min(t, 1 - 1e-10); first the non-ignored ground truths in pooled order, then -- only if none of them matched -- the ignored ones;
 *   matched non-crowd ground truths are skipped; >= keeps the LATER (in pooled order) of equal IoUs.  An unmatched detection whose area
 *   lies outside the range is ignored.
 * Effects: npig[0, a] += the frame's ground truths of all labels not ignored in range a (npig is [1,4]); *cursor += the kept detections
 * (one atomic add; slots past record_capacity are counted, not written); records as frcnn_coco_eval_update writes them with label = 0
 * for every record and rank = the pooled rank; the defined order of the set is (score descending, image_id ascending, rank ascending).
 * frcnn_coco_eval_accumulate with C = 2 (K = 1) accumulates them for any three maxDets.  The error word is that of
 * frcnn_coco_eval_update; a frame with any bit is not recorded.
 * Limits (FRCNN_ERR_UNSUPPORTED otherwise): 2 <= C <= 256, 1 <= det_capacity <= (C-1) * 2048, 1 <= gt_capacity <= 1024, 1 <= T <= 16,
 * 1 <= max_det <= 2048.  boxes 16-byte aligned, gt_boxes and gt_area 8-byte aligned.  workspace:
 * frcnn_workspace_bytes(FRCNN_OP_COCO_EVAL_POOLED, det_capacity, gt_capacity) bytes, ANY content between calls (every word the second
 * launch reads, and every flag word it ORs into, is written by the first launch of the same call), not shared with a call that may run at
 * the same time. */
int frcnn_coco_eval_update_pooled(const float *boxes /*[D,4]*/, const int32_t *labels /*[D]*/, const float *scores /*[D]*/,
                                  const int32_t *count_dev, int64_t det_capacity, const double *gt_boxes /*[G,4] pixel xywh*/,
                                  const double *gt_area /*[G]*/, const int32_t *gt_labels /*[G]*/, const uint8_t *gt_iscrowd /*[G]*/,
                                  const int32_t *n_gt_dev, int64_t gt_capacity, const int32_t *frame_dev /*[3]: w, h, image_id*/,
                                  const double *thresholds_dev /*[T]*/, int T, int C, int max_det, int64_t *npig /*[1,4]*/, float *rec_score,
                                  int32_t *rec_label, int32_t *rec_image, int32_t *rec_rank, uint32_t *rec_flags /*[record_capacity,4]*/,
                                  int64_t record_capacity, int64_t *cursor /*[1]*/, int32_t *error_word /*[1]*/, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* ---- detection evaluators: the image ledger and the merge of shards across ranks (test.py:60-128, evaluation/coco_eval.py:46-49,161-190) -- */
/* One ledger row per frame, in one launch on the stream of the update before it (frcnn_eval_update or frcnn_coco_eval_update), with no
 * host sync (graph-capturable).  Row *led_count receives image_id = frame_dev[2], the record slots [*snap_cursor, *cursor) the frame took
 * and delta[w] = int32(counter[w] - snap_counter[w]) for the counter_words words of the protocol's counter (VOC: C-1, COCO: 4 (C-1));
 * then *snap_cursor = *cursor, snap_counter = counter and *led_count += 1.  The snapshots belong to the caller and start at zero with
 * the store.  A full ledger writes no row, keeps counting and sets *error_word |= 16.
 * Limits: image_capacity >= 1; 1 <= counter_words <= 1020 (FRCNN_ERR_UNSUPPORTED otherwise). */
int frcnn_eval_ledger_append(const int32_t *frame_dev /*[3]: w, h, image_id*/, const int64_t *cursor /*[1]*/, const int64_t *counter /*[counter_words]*/,
                             int64_t counter_words, int64_t *snap_cursor /*[1]*/, int64_t *snap_counter /*[counter_words]*/, int32_t *led_image,
                             int64_t *led_range /*[image_capacity,2]*/, int32_t *led_delta /*[image_capacity,counter_words]*/,
                             int64_t image_capacity, int64_t *led_count /*[1]*/, int32_t *error_word /*[1]*/, void *stream);
/* Merges W shards of one evaluator class into a destination store, whose previous content is replaced: the reference's merge
 * (evaluation/coco_eval.py:161-190: all_gather, then np.unique(img_ids, return_index=True)).  Occurrences are ordered (shard, ledger
 * row); an occurrence is KEPT iff no earlier occurrence has its image_id -- duplicates inside one shard are dropped too; every int32 is
 * a legal id.  Shards arrive as one padded buffer per column, [W, shard capacity, ...] (the result of an all-gather as it is); the live
 * counts sh_n_records / sh_n_images (int64 [W], clipped to the capacities) and sh_error are read on the device: no host sync, a fixed
 * number of launches whatever the data, graph-capturable.  A row's range is clipped to its shard's live records before it is used;
 * the ranges of a shard ascend, as frcnn_eval_ledger_append writes them.
 * Effects: the records of kept occurrences in (shard, slot) order, all five columns bit for bit (slots past record_capacity are counted,
 * not written); the kept ledger rows in the same order with rebased ranges (rows past image_capacity are counted, not written);
 * counter = the sum of the kept rows' delta; *cursor = the kept records; *led_count = the kept rows; *error_word = the OR of sh_error,
 * | 16 when the kept rows exceed image_capacity, | 32 when a shard's count exceeds its capacity (it had lost some); *snap_cursor / snap_counter follow, so that updates may go on.
 * flags_width: 1 (VOC) or 4 (COCO) words per record.  FRCNN_ERR_INVALID_ARG: a NULL pointer, a negative capacity, a
 * shard_record_capacity that is no multiple of 4, another flags_width, record columns that are not 16-byte aligned, a destination
 * buffer that overlaps a shard buffer, the workspace or another destination buffer.  FRCNN_ERR_UNSUPPORTED: W outside 1 .. 64,
 * counter_words outside 1 .. 1020, W * shard_record_capacity >= 2^31 - 4096, W * shard_image_capacity >= 2^30.  FRCNN_ERR_WORKSPACE:
 * fewer than frcnn_workspace_bytes(FRCNN_OP_EVAL_MERGE, W * shard_record_capacity, W * shard_image_capacity) bytes (any content). */
int frcnn_eval_merge(int W, int64_t shard_record_capacity, int64_t shard_image_capacity, int flags_width, int64_t counter_words,
                     const float *sh_score, const int32_t *sh_label, const int32_t *sh_image, const int32_t *sh_order, const uint32_t *sh_flags,
                     const int32_t *sh_led_image, const int64_t *sh_led_range, const int32_t *sh_led_delta, const int64_t *sh_n_records /*[W]*/,
                     const int64_t *sh_n_images /*[W]*/, const int32_t *sh_error /*[W]*/, float *rec_score, int32_t *rec_label,
                     int32_t *rec_image, int32_t *rec_order, uint32_t *rec_flags, int64_t record_capacity, int32_t *led_image,
                     int64_t *led_range, int32_t *led_delta, int64_t image_capacity, int64_t *counter, int64_t *cursor /*[1]*/,
                     int64_t *led_count /*[1]*/, int32_t *error_word /*[1]*/, int64_t *snap_cursor /*[1]*/, int64_t *snap_counter,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- input stage in front of the path ------------------------------------------------------
 * One uint8 HWC RGB frame in HBM -> [hflip] -> PIL-bilinear resize to (oh, ow) -> /255 -> (x - mean) / std -> float CHW
 * [3, pad_h, pad_w], zero outside (oh, ow).  Replaces T.RandomHorizontalFlip / T.Resize(800, max 1333) / T.ToTensor /
 * T.Normalize (new_datasets/transforms.py:57-132,238-281; new_datasets/build.py:20-33, datasets/build.py:10-24) and the
 * pad-to-32 collate (new_datasets/coco_dataset.py:49-66).  Bit-identical to Pillow's 8-bit resampler.  mean/std: host,
 * 3 floats.  out_u8 (optional, [oh, ow, 3]) receives the resized uint8 frame; either output may be NULL, not both.  */
int frcnn_preprocess_image(const uint8_t *src_hwc, int h, int w, int flip, int oh, int ow, int pad_h, int pad_w,
                           const float *mean_host, const float *std_host, float *out_chw, uint8_t *out_u8,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Boxes xyxy in source pixels -> hflip (transforms.py:64-68) -> x resize ratios (:113-117) -> / resized (w, h) (:276-280),
 * i.e. the normalised boxes the model takes.  binary32 throughout, like the reference's tensors.                   */
int frcnn_preprocess_boxes(const float *boxes, int64_t n, int w, int h, int flip, int ow, int oh, float *out, void *stream);

/* ---- mosaic augmentation (--mosaic_transform, config.py:16) -------------------------------------------------------
 * Four uint8 HWC RGB frames in HBM -> one [2*size, 2*size, 3] uint8 canvas and one compacted box / label list.  Replaces load_mosaic
 * (datasets/mosaic_transform.py:39-95; called from datasets/voc_dataset.py:145-156 and datasets/coco_dataset.py:154-157) without its
 * choice of frames: per tile k = 0..3
 *   Resize(size, max_size)     resize_, datasets/transforms_.py:61-127: Pillow's 8-bit bilinear resize to H1 x W1, boxes * (W1/w, H1/h)
 *   RandomSizeCrop's crop_     transforms_.py:150-178 with the CALLER's region (i, j, h, w) (the draw of :284-286 is the caller's): boxes
 *                              - (j, i), min (w, h), clamp at 0; kept when both sides > 0 and (cw*ch) / (bw*bh) > 0.3; when NO box is
 *                              kept (a tile without boxes included) the tile is the uncropped H1 x W1 frame with ALL its boxes (:174-176)
 *   Resize((size, size))       a second Pillow resize of the cropped image as an image of its own, boxes * (size/w, size/h)
 *   shift_mosaic_boxes         mosaic_transform.py:7-12,82-85: + (0,0), (size,0), (0,size), (size,size)
 *   get_concat_h/v_cut_center  mosaic_transform.py:15-26,88-93: the four size x size tiles side by side; boxes, labels in tile order
 * Bit-identical to Pillow and to the reference's binary32 box arithmetic.  The crop decision is taken on the device and never read
 * back: a fixed six launches, no allocation, capturable.
 *   src_hw [4][2] (h, w) and regions [4][4] are HOST arrays, read during the call.  max_size <= 0: no cap.  tile_offsets [5] HOST:
 *   tile k owns rows [tile_offsets[k], tile_offsets[k+1]) of boxes / labels; N = tile_offsets[4] (0 is legal: every tile falls back).
 *   boxes [N,4] pixel xyxy of the source frames, labels [N]; boxes_out [N,4], labels_out [N]: the first *count_dev rows live, in tile
 *   order and each tile's own order, zeros behind them.  boxes and boxes_out 16-byte aligned, not overlapping.  fallback_dev [4]: 1
 *   where the tile was not cropped.  workspace: frcnn_mosaic_workspace(src_hw, size, max_size) bytes (0 for shapes it refuses).
 * FRCNN_ERR_INVALID_ARG, before anything is launched: a NULL pointer; a side of a source or resized frame, or 2 * size, of 2^15 or
 * more; a region outside its resized frame or with h < 1 or w < 1; offsets that do not start at 0 or decrease.  FRCNN_ERR_WORKSPACE: a
 * short workspace.  */
size_t frcnn_mosaic_workspace(const int32_t *src_hw, int size, int max_size);
int frcnn_mosaic(const uint8_t *const src_hwc[4], const int32_t *src_hw, int size, int max_size, const int32_t *regions,
                 const float *boxes, const int64_t *labels, const int32_t *tile_offsets, uint8_t *canvas, float *boxes_out,
                 int64_t *labels_out, int32_t *count_dev, uint8_t *fallback_dev, void *workspace, size_t workspace_bytes, void *stream);

/* ---- photometric distortion and zoom-out (the richer training recipe, datasets/build.py:28-42) ---------------------------------
 * frcnn_photometric replaces photometric_distort_ (datasets/transforms_.py:38-58; RandomPhotoDistortion :240-247, whose coin and draws
 * stay with the caller) for one uint8 HWC RGB frame in HBM: [h, w, 3] -> [h, w, 3].  Bit-identical to Pillow 12.2 for the calls
 * torchvision's PIL backend makes:
 *   blend(a, b, alpha)  Image.blend: alpha binary32, t = a + alpha * (b - a) rounded after each operation; alpha in [0, 1]: (uint8) t,
 *                       otherwise 0 for t <= 0, 255 for t >= 255, else (uint8) t.  a = the degenerate byte, b = the image byte
 *   brightness (op 0)   a = 0                         saturation (op 2)   a = the pixel's L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *   contrast   (op 1)   a = int(sum(L) / count + 0.5) in binary64 over the image AS IT STANDS when contrast is applied (exact 64-bit sum)
 *   hue        (op 3)   convert("HSV"), H += shift mod 256, convert("RGB") in Pillow's mixed binary32 / binary64 arithmetic; a shift of
 *                       0 still goes through both conversions and is not the identity
 * plan_dev: int32[8] in DEVICE memory, read by the kernels (a captured graph sees what the buffer holds at each replay): four slots
 * (op, param) applied in order, every op on the uint8 result of the one before.  param: the binary32 bits of alpha (ops 0-2), the hue
 * shift 0..255 (op 3: uint8(int32(factor * 255)), the product in binary64, truncated toward zero).  A slot whose op is outside 0..3
 * is skipped; so is an op from its second appearance on.  No host synchronisation and two launches whatever the plan says.
 * out must not overlap src.  src, out 4-byte aligned.  workspace: frcnn_photometric_workspace(h, w) bytes (0 for shapes it refuses),
 * 8-byte aligned, any content: nothing of an earlier call is read.
 * FRCNN_ERR_INVALID_ARG, before anything is launched: a NULL pointer, a side outside 1 .. 32767, a misaligned pointer, out overlapping
 * src.  FRCNN_ERR_WORKSPACE: a short workspace.  */
size_t frcnn_photometric_workspace(int h, int w);
int frcnn_photometric(const uint8_t *src_hwc, int h, int w, const int32_t *plan_dev, uint8_t *out_hwc, void *workspace,
                      size_t workspace_bytes, void *stream);
/* frcnn_zoom_out replaces zoom_out_ (datasets/transforms_.py:130-147; RandomZoomOut :291-299, whose coin and draws stay with the
 * caller): a [new_h, new_w, 3] canvas filled with the frame's per-channel MEDIAN (the reference's `mean_color` is
 * ImageStat.Stat(image)._getmedian(): the first level whose cumulative count exceeds count / 2), the frame pasted at (left, top), boxes
 * + float32(left, top, left, top).  new_h = int(scale * h), new_w = int(scale * w), top and left are the CALLER's host integers: shapes
 * stay host-known.  The histogram and the median stay on the device: three launches (kernels only), capturable.  n = 0 is legal
 * (boxes and boxes_out may then be NULL).  src, canvas 4-byte aligned and not overlapping; boxes, boxes_out 16-byte aligned.
 * workspace: frcnn_zoom_out_workspace(h, w, new_h, new_w) bytes (0 for shapes it refuses), 4-byte aligned, any content.
 * FRCNN_ERR_INVALID_ARG, before anything is launched: a NULL pointer, n < 0, a side of the frame or the canvas outside 1 .. 32767, a
 * canvas smaller than the frame, top outside 0 .. new_h - h or left outside 0 .. new_w - w, a misaligned pointer, the canvas
 * overlapping src.  FRCNN_ERR_WORKSPACE: a short workspace.  */
size_t frcnn_zoom_out_workspace(int h, int w, int new_h, int new_w);
int frcnn_zoom_out(const uint8_t *src_hwc, int h, int w, int new_h, int new_w, int top, int left, const float *boxes /*[n,4] xyxy*/, int64_t n,
                   uint8_t *canvas, float *boxes_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- crop, with the resize in front of it (the multi-scale recipe sketched in datasets/build.py:27-39) -----------------------------
 * frcnn_resize_crop replaces resize (new_datasets/transforms.py:76-132) followed by crop (:16-56; the region is the CALLER's: RandomCrop
 * :162-168, RandomSizeCrop :171-180 and CenterCrop :183-192 only choose it) for one uint8 HWC RGB frame in HBM:
 *   image  Pillow's 8-bit bilinear resize to H1 x W1 (horizontal pass, uint8, vertical pass), of which only the region (i, j, ch, cw) is
 *          computed -> out_hwc [ch, cw, 3], the bytes of F.resize then F.crop on a PIL image.  (H1, W1) == (h, w): a plain crop, a byte
 *          copy of the region (Pillow returns a copy for an equal size).
 *   boxes  [n, 4] pixel xyxy of the SOURCE frame: * float32(W1/w, H1/h) (the ratios formed in double, :111-117), - (j, i, j, i), min with
 *          (cw, ch) (NaN propagates), clamp at 0 (NaN stays) (:29-32); area_out = (x2 - x1) * (y2 - y1) (:33); a row is kept when
 *          x2 > x1 and y2 > y1 (:48-49: a NaN box is dropped).  boxes / labels / area / iscrowd of the kept rows are compacted in input
 *          order into boxes_out [n, 4], labels_out [n], area_out [n], iscrowd_out [n], zeros behind them; *count_dev = their number.
 *          There is no area INPUT: crop replaces every area by that of the clipped box, so the product resize forms (:122) is never
 *          seen.  area_out may be NULL; iscrowd and iscrowd_out are given together or not at all.
 *   count_in_dev  NULL, or a device int32: only the first min(max(*count_in_dev, 0), n) rows are live (a list that an earlier device
 *          stage compacted); the rows behind them are ignored.
 * Binary32 throughout, operation for operation.  This crop always crops (datasets/transforms_.py:crop_, which may hand back the uncropped
 * frame, is frcnn_mosaic's), so every shape is the host's.  No host synchronisation; four launches (two for a plain crop), whatever the
 * boxes say; capturable.  n = 0 is legal (the list pointers may then be NULL).  boxes, boxes_out 16-byte aligned; no output overlaps
 * its input.  workspace: frcnn_resize_crop_workspace(h, w, H1, W1, ch, cw) bytes (0 for shapes it refuses), 4-byte aligned, any content.
 * FRCNN_ERR_INVALID_ARG, before anything is launched: n < 0; a NULL pointer; a side of the frame or the resized frame outside
 * 1 .. 32767; ch < 1 or cw < 1; a region that is not inside the resized frame (PIL would pad it with black; no recipe of the reference
 * draws one); a misaligned or overlapping list.  FRCNN_ERR_WORKSPACE: a short workspace.  */
size_t frcnn_resize_crop_workspace(int h, int w, int H1, int W1, int ch, int cw);
int frcnn_resize_crop(const uint8_t *src_hwc, int h, int w, int H1, int W1, int i, int j, int ch, int cw, const float *boxes,
                      const int64_t *labels, const int64_t *iscrowd, int64_t n, const int32_t *count_in_dev, uint8_t *out_hwc,
                      float *boxes_out, int64_t *labels_out, float *area_out, int64_t *iscrowd_out, int32_t *count_dev,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- optimizer: SGD with momentum and weight decay, hyper-parameters in device memory -----------------------------------------------
 * The three entry points replace torch.optim.SGD as main.py:58-61 constructs it (lr, momentum, weight_decay; dampening 0, no Nesterov,
 * maximize=False) and train.py:35-37 steps it, for fp32 dense tensors, in place on parameter and momentum:
 *   d  = wd != 0 ? fma(wd, p, g) : g          (no product with a zero weight decay)
 *   m' = (the tensor's first update, or mu == 0) ? d : round(mu * m) + d
 *   p' = fma(-lr, m', p)
 * every fma rounded once: the bits of torch.optim.SGD on the CPU (tests/golden/sgd.npz).  With mu == 0 the momentum is neither read nor
 * written and the tensor's born word is left alone (torch keeps no buffer then).
 *   hyper  float[n_groups][4] = (lr, momentum, weight_decay, unused) in DEVICE memory, 16-byte aligned, read by the kernel at run time: a
 *          captured graph applies whatever the block holds at each replay.
 *   born   int32[n_tensors] in DEVICE memory: 0 = the tensor's momentum has never been written (its content is then not read).  Read by
 *          the update, set by a second small launch behind it.
 *   skip   NULL, or a device int32: when non-zero the step changes nothing (parameters, momentum, born words).
 *   table  frcnn_sgd_table_bytes(n_tensors, numel_host) bytes, filled on the HOST by frcnn_sgd_table_build_host from arrays of DEVICE
 *          pointers (parameter, gradient, momentum), element counts and group indices, then uploaded by the caller to 16-byte aligned
 *          device memory.  It holds one row per tensor and one entry per 8192-element chunk; *n_chunks_host is the number of entries.
 *          Pointers need 4-byte alignment only; a tensor whose three pointers are 16-byte aligned is moved with 16-byte accesses.
 * frcnn_sgd_table_bytes: 0 for counts the builder refuses.  frcnn_sgd_table_build_host, FRCNN_ERR_INVALID_ARG: a NULL array, n_tensors
 * outside 1 .. 65536, n_groups outside 1 .. 1024, a negative size, a NULL or misaligned pointer in a row, a group index outside
 * 0 .. n_groups - 1, overlapping parameter and momentum ranges (of one row or of two), a gradient overlapping either;
 * FRCNN_ERR_WORKSPACE: a short table.  frcnn_sgd_step (main.py:58-61, train.py:35-37): two launches whatever the number and sizes of the
 * tensors, no host synchronisation, capturable.  FRCNN_ERR_INVALID_ARG before anything is launched: a NULL table / hyper / born, bad
 * counts, a misaligned pointer; FRCNN_ERR_WORKSPACE: table_bytes below what n_tensors and n_chunks need.  */
size_t frcnn_sgd_table_bytes(int n_tensors, const int64_t *numel_host);
int frcnn_sgd_table_build_host(int n_tensors, const void *const *params_host, const void *const *grads_host, const void *const *moms_host,
                               const int64_t *numel_host, const int32_t *group_host, int n_groups, void *table_host, size_t table_bytes,
                               int32_t *n_chunks_host);
int frcnn_sgd_step(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                   const int32_t *skip, void *stream);

/* ---- optimizer: global gradient norm, clip coefficient and non-finite skip word, all in device memory ---------------------------------
 * What torch.nn.utils.clip_grad_norm_(parameters, max_norm) in front of optimizer.step() (train.py:35-37) computes, without its pass
 * that rewrites the gradients and without a host read: frcnn_grad_norm measures the L2 norm of every gradient of an SGD table (the
 * table frcnn_sgd_table_build_host made: rows and chunk map are reused as they are) and counts the non-finite elements, and leaves a clip
 * coefficient and a skip word in a device state block; frcnn_sgd_step_scaled is frcnn_sgd_step with every gradient element multiplied by
 * a device float (that coefficient) on its way into the rule: round(g * coef), the bits of torch's in-place g.mul_(coef) followed by
 * torch.optim.SGD.  The gradients are never written.
 *
 * The state block: 64 bytes of DEVICE memory, 16-byte aligned.  max_norm and flags are inputs, written by the caller outside any graph;
 * steps and skipped_steps are running counters the caller zeroes once; everything else is rewritten by every call. */
typedef struct {
    float max_norm;          /*  0  in   the clip threshold (read when FRCNN_GRAD_NORM_CLIP is set) */
    uint32_t flags;          /*  4  in   FRCNN_GRAD_NORM_CLIP | FRCNN_GRAD_NORM_SKIP_NONFINITE */
    double sumsq;            /*  8  out  the sum of the squares, binary64, in the order below */
    float norm;              /* 16  out  (float)sqrt(sumsq), both correctly rounded */
    float coef;              /* 20  out  clip set: c = max_norm / (norm + 1e-6f) in binary32, c > 1 ? 1 : c (a NaN stays NaN); else 1 */
    int32_t skip;            /* 24  out  1 or 0: (SKIP_NONFINITE set and nonfinite != 0) or (user_guard given and *user_guard != 0) */
    int32_t nonfinite;       /* 28  out  elements whose exponent field is all ones (inf, NaN), saturating at INT32_MAX */
    int32_t steps;           /* 32  i/o  += 1 per call */
    int32_t skipped_steps;   /* 36  i/o  += skip per call */
    int32_t reserved[6];     /* 40       not touched */
} frcnn_grad_norm_state;
#define FRCNN_GRAD_NORM_CLIP 1u
#define FRCNN_GRAD_NORM_SKIP_NONFINITE 2u
#define FRCNN_GRAD_NORM_FINISH_THREADS 1024
/* The summation order is part of the contract: sumsq depends on the gradient VALUES and on each element's position in its tensor only --
 * never on pointer alignment, on which load path ran, on residency or on timing.  No atomics; no workgroup waits on another.
 *   element  every element x is widened to binary64 and squared there (exact: 48 significant bits).
 *   chunk    chunk c of a tensor holds its elements [8192 c, 8192 c + n), n <= 8192, element i of the chunk at position i.  One workgroup
 *            of 256 threads.  Thread t, t = (i / 4) % 256, owns the elements i with that t; it keeps four binary64 accumulators, one per
 *            e = i % 4, each starting at +0 and taking its squares in increasing i (j = i / 1024 = 0 .. 7); then a = (a0 + a1) + (a2 + a3).
 *   wave     the 64 threads of a wave (t / 64) combine by an xor butterfly: for d = 32, 16, 8, 4, 2, 1: a[t] = a[t] + a[t ^ d] (every
 *            lane ends with the same bits).
 *   block    partial[c] = ((w0 + w1) + w2) + w3, the four waves in wave order; stored with a plain store, the chunk's int32 count of
 *            non-finite elements beside it.
 *   finish   one workgroup of T = FRCNN_GRAD_NORM_FINISH_THREADS threads over the n_chunks partials in map order (tensor by tensor,
 *            chunk by chunk): thread t starts at +0 and adds partials t, t + T, t + 2T, ... in that order; then the butterfly above
 *            inside each of the 16 waves; then the waves in wave order, (((w0 + w1) + w2) + ...) + w15.  Counts: the same tree in int64.
 * Finite gradients cannot overflow the sum (at most 2^56 squares below 2^256 each); a norm above FLT_MAX becomes +inf and coef 0, as torch's
 * fp32 norm does.  tests/grad_norm_ref.py restates all of it in numpy.
 *
 * frcnn_grad_norm_workspace_bytes: bytes for n_chunks partials and counts (at least 16); 0 for a negative count.  The workspace is
 * 16-byte aligned device memory, fully rewritten by every call.  frcnn_grad_norm (train.py:35-37): two launches whatever the tensors
 * are, no host synchronisation, capturable; n_chunks == 0 (every tensor empty) still runs the finish (norm 0).  user_guard: NULL, or a
 * device int32 OR-ed into the skip word.  frcnn_sgd_step_scaled (train.py:35-37): frcnn_sgd_step's arguments and refusals, and
 * grad_scale, a device float, 4-byte aligned, not NULL -- &state->coef.  Pass &state->skip as `skip` to either step function.
 * FRCNN_ERR_INVALID_ARG before anything is launched: a NULL table / state / workspace, n_tensors outside 1 .. 65536, a negative
 * n_chunks, a table, state or workspace that is not 16-byte aligned, a user_guard that is not 4-byte aligned; FRCNN_ERR_WORKSPACE: a
 * table shorter than n_tensors and n_chunks need, a workspace shorter than frcnn_grad_norm_workspace_bytes(n_chunks). */
size_t frcnn_grad_norm_workspace_bytes(int n_chunks);
int frcnn_grad_norm(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_grad_norm_state *state, const int32_t *user_guard,
                    void *workspace, size_t workspace_bytes, void *stream);
int frcnn_sgd_step_scaled(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                          const int32_t *skip, const float *grad_scale, void *stream);

/* ---- optimizer: gradient accumulation over a window of K frames, the window's state in device memory -----------------------------------
 * The reference trains on one frame per update (train.py:31-37: forward, loss.backward(), optimizer.step()) and has no accumulation; the
 * usual recipe for a larger effective batch is K backward passes of loss / K summed into .grad and ONE optimizer step.  Here the sum is
 * formed by a multi-tensor launch whose decision -- write (a window's first frame), add (a later frame) or leave the frame out (a frame
 * without boxes, whose gradients are NaN) -- is read from device memory, so one captured graph serves every micro-step of every window.
 *
 * The state block: 64 bytes of DEVICE memory, 16-byte aligned.  window is written by the caller outside any graph; the caller zeroes the
 * rest once.  frcnn_grad_accumulate only READS the block; frcnn_grad_accum_advance is the one writer. */
typedef struct {
    int32_t window;          /*  0  in   K >= 1, written by the caller outside any graph */
    int32_t phase;           /*  4  i/o  0 .. K-1: the micro-step inside the window */
    int32_t live;            /*  8  i/o  frames of this window that contributed */
    int32_t hold;            /* 12  out  written by advance: 1 unless this call closed a window with live > 0 */
    int32_t windows;         /* 16  i/o  windows closed */
    int32_t frames;          /* 20  i/o  advance calls */
    int32_t dropped;         /* 24  i/o  frames left out (frame_skip != 0) */
    int32_t reserved[9];     /* 28       not touched */
} frcnn_grad_accum_state;
#define FRCNN_GRAD_ACCUM_ROWS 96
/* frcnn_grad_accumulate, fp32 only.  p = state->phase and s = frame_skip ? *frame_skip : 0 are read on the device, once per workgroup;
 * then, for every element of every tensor:
 *
 *                              s == 0                                 s != 0
 *   p == 0                     acc = src   (acc is NOT read)          acc = +0.0f   (neither is read)
 *   0 < p < window             acc = acc + src, rounded once          nothing is read or written
 *   p outside 0 .. window-1    nothing is touched                     nothing is touched
 *
 * One rounding per add: the bits of torch's grad.add_(g).  Only acc is written.  src_host / acc_host / numel_host are HOST arrays of
 * n_tensors device pointers and element counts (the sources are typically autograd's gradient tensors, whose addresses exist only inside
 * a capture, where nothing can be uploaded): the library hands them to its kernel BY VALUE in the kernel arguments, which a graph node
 * stores, at most FRCNN_GRAD_ACCUM_ROWS rows per launch (frcnn_grad_accum_rows_per_launch returns that number).  The number of launches
 * is ceil(n_tensors / rows per launch) minus the launches whose rows are all empty: it depends on the tensor list only, never on data.
 * One workgroup of 256 threads per 8192-element chunk of a tensor; 16-byte accesses when both pointers of a row are 16-byte aligned,
 * dword accesses for such a row's tail and for all of any other row.  No atomics, no workgroup waits on another.
 *
 * frcnn_grad_accum_advance, one small launch, is the window's bookkeeping (a call of its own because one micro-step may make several
 * frcnn_grad_accumulate calls, which must all see the same phase):
 *   1. frames += 1, dropped += (s != 0), live += (s == 0)
 *   2. phase + 1 == window:  hold = (live == 0), windows += 1, phase = 0, live = 0
 *   3. otherwise:            hold = 1, phase += 1
 * (a block whose phase lies outside 0 .. window-1 is not ours: nothing is written).  Pass &state->hold as the `skip` word of
 * frcnn_sgd_step, or as the user_guard of frcnn_grad_norm: an update attempted after every frame then happens exactly when a window
 * with at least one live frame has closed.  A frame that is left out contributes zero; the divisor of the mean stays K (the caller
 * seeds its backward with 1 / K).  tests/grad_accum_ref.py restates both functions in numpy.
 *
 * Both make no host synchronisation and are capturable.  FRCNN_ERR_INVALID_ARG before anything is launched: a NULL array or state,
 * n_tensors outside 1 .. 65536, a negative size or one above 2^40, a NULL pointer in a row or one that is not 4-byte aligned, a state that
 * is not 16-byte aligned, a frame_skip that is not 4-byte aligned, two overlapping acc ranges, a src range that overlaps any acc range.
 * Tensors of size 0 are legal rows; if every tensor is empty nothing is launched. */
int frcnn_grad_accum_rows_per_launch(void);
int frcnn_grad_accumulate(int n_tensors, const void *const *src_host, void *const *acc_host, const int64_t *numel_host,
                          const frcnn_grad_accum_state *state, const int32_t *frame_skip, void *stream);
int frcnn_grad_accum_advance(frcnn_grad_accum_state *state, const int32_t *frame_skip, void *stream);

/* ---- optimizer: exponential moving average of the weights, in device memory, fused into the SGD step, swappable in place ----------------
 * The reference evaluates and checkpoints the raw weights (train.py:75-85) and keeps no average: this is defined by this project and
 * pinned to torch.  Per element, p' the parameter after this update, e its average ("shadow"), w the float32 weight of this update:
 *   d  = round(p' - e)
 *   e' = |w| < 0.5 ? fma(w, d, e) : fma(round(w - 1), d, p')          every fma rounded once
 * the bits of torch._foreach_lerp_([e], [p'], w) on the CPU, which torch.optim.swa_utils.get_ema_multi_avg_fn runs
 * (tests/golden/ema.npz).  The weight follows a schedule evaluated in binary64, n the number of updates applied so far:
 *   decay_t = warm-up ? min(decay, (1 + n) / (10 + n)) : decay          w = (float)(1.0 - decay_t)
 * The caller writes w for n = 0; after every applied update the device computes the next one (one thread, binary64).
 *
 * The state block: 64 bytes of DEVICE memory, 16-byte aligned.  decay and flags are inputs, written once by the caller outside any graph,
 * with num_updates and w for the starting n; the counters are zeroed by the caller.  The advance launch (one thread) is the only writer
 * of num_updates, w, skipped and refused; frcnn_ema_swap (one thread of it) is the only writer of swapped. */
typedef struct {
    double decay;            /*  0  in   0 <= decay < 1 */
    int64_t num_updates;     /*  8  i/o  n: updates applied so far */
    float w;                 /* 16  i/o  the weight of the NEXT update: (float)(1.0 - decay_t(n)) */
    uint32_t flags;          /* 20  in   FRCNN_EMA_WARMUP */
    int32_t swapped;         /* 24  i/o  1 while the parameters hold the averaged weights (frcnn_ema_swap toggles it) */
    int32_t skipped;         /* 28  i/o  updates left out because the skip word was set */
    int32_t refused;         /* 32  i/o  updates (fused: whole steps) left out because swapped was set */
    int32_t reserved[7];     /* 36       not touched */
} frcnn_ema_state;
#define FRCNN_EMA_WARMUP 1u
/* The table: frcnn_ema_table_bytes(n_tensors, numel_host) bytes, filled on the HOST by frcnn_ema_table_build_host from arrays of DEVICE
 * pointers (parameter, shadow) and element counts, then uploaded by the caller to 16-byte aligned device memory: one row per tensor, one
 * map entry per 8192-element chunk -- for the same sizes entry for entry the SGD table's map.  Pointers need 4-byte alignment only; a
 * row whose two pointers are 16-byte aligned is moved with 16-byte accesses, any other with dword accesses for its whole length.
 * frcnn_ema_table_bytes: 0 for counts the builder refuses.  frcnn_ema_table_build_host, FRCNN_ERR_INVALID_ARG: a NULL array, n_tensors
 * outside 1 .. 65536, a negative size or one above 2^40, a NULL pointer in a row or one that is not 4-byte aligned, any overlap among
 * the parameter and shadow ranges (of one row or of two); FRCNN_ERR_WORKSPACE: a short table.
 *
 * frcnn_ema_update: the stand-alone form, behind any optimizer: two launches, no host synchronisation, capturable.  Every workgroup of
 * the first reads w, swapped and *skip (NULL allowed); with neither set it applies the rule to its chunk; only e is written.  The
 * second, one thread, is the bookkeeping:
 *   swapped != 0:  refused += 1            else *skip != 0:  skipped += 1            else:  num_updates += 1, w = the weight for the new n
 * frcnn_ema_swap: one launch, capturable, not gated by any skip word: p and e exchanged element for element in place, swapped toggled.
 * No address changes: graphs captured on the parameters run on the averaged weights between two swaps.
 * frcnn_sgd_step_ema: frcnn_sgd_step (grad_scale NULL) or frcnn_sgd_step_scaled (grad_scale given) with the average fused in: the update
 * kernel loads e behind computing p', applies the rule and stores e' -- 28 B per element against 32 B in two passes; then the born
 * launch, then the bookkeeping above: three launches.  It reads ONE skip word for all of it.  While swapped is set the WHOLE step changes
 * nothing -- parameters, momentum, born words, average -- and is counted in refused: training on the averaged weights would corrupt both
 * sets.  The EMA table must be built over the SGD table's parameters, in its row order; a row takes the 16-byte path only when the SGD
 * row's three pointers and the shadow are 16-byte aligned; a workgroup whose two rows disagree on parameter or size touches nothing.
 * FRCNN_ERR_INVALID_ARG before anything is launched: a NULL table or state, bad counts, a table or state that is not 16-byte aligned,
 * a skip word that is not 4-byte aligned, and for the fused form frcnn_sgd_step's refusals; FRCNN_ERR_WORKSPACE: a short table. */
size_t frcnn_ema_table_bytes(int n_tensors, const int64_t *numel_host);
int frcnn_ema_table_build_host(int n_tensors, const void *const *params_host, const void *const *shadows_host, const int64_t *numel_host,
                               void *table_host, size_t table_bytes, int32_t *n_chunks_host);
int frcnn_ema_update(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_ema_state *state, const int32_t *skip,
                     void *stream);
int frcnn_ema_swap(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_ema_state *state, void *stream);
int frcnn_sgd_step_ema(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                       const int32_t *skip, const float *grad_scale, const void *ema_table, size_t ema_table_bytes, frcnn_ema_state *ema_state,
                       void *stream);

/* ---- training telemetry: per-tensor statistics over an SGD table, and a journal of scalars, all in device memory -------------------------
 * The reference's loop prints its losses and the lr every vis_step steps (train.py:39-72) from host floats (loss.item(): a sync per
 * step).  A graph-replayed run keeps its record on the device instead: frcnn_tensor_stats measures every tensor of an SGD table (the table
 * frcnn_sgd_table_build_host made: rows and chunk map reused as they are, born the optimizer's born words), frcnn_journal_append keeps one
 * row of scalars per call in a ring.  Both are defined by this project; what the journal's totals reproduce of the reference's
 * SmoothedValue (util/misc.py:27-86) is said below.  Gradients, parameters and momenta are only read.
 *
 * One row per tensor, 64 bytes, rows[n_tensors] in DEVICE memory, 16-byte aligned, rewritten by every MEASURING call: */
typedef struct {
    double g_sumsq;          /*  0  the sum of the squares of the gradient, binary64, in the order below */
    double p_sumsq;          /*  8  ... of the parameter */
    double m_sumsq;          /* 16  ... of the momentum; +0 when m_read == 0 */
    float g_absmax;          /* 24  max |g|: the `>` comparison from +0, so a NaN never wins and an inf does; order-free */
    float p_absmax;          /* 28  max |p| */
    int32_t g_nonfinite;     /* 32  gradient elements whose exponent field is all ones (inf, NaN), saturating at INT32_MAX */
    int32_t p_nonfinite;     /* 36  ... parameter elements */
    int32_t m_read;          /* 40  1: born[tensor] != 0 and the tensor has elements, its momentum was read; 0: not one byte of it was loaded */
    int32_t reserved[5];     /* 44  written as zero */
} frcnn_tensor_stats_row;
/* The state block: 64 bytes of DEVICE memory, 16-byte aligned.  every is an input, written by the caller outside any graph; the caller
 * initialises tick = 0, measured_tick = -1, measures = 0, first_nonfinite_g = first_nonfinite_p = -1 once. */
typedef struct {
    int32_t every;             /*  0  in   N >= 1: the call measures when tick % N == 0 */
    int32_t tick;              /*  4  i/o  calls so far; (tick + 1) & INT32_MAX per call */
    int32_t measured_tick;     /*  8  out  the tick whose data the rows hold; the caller's -1 before the first */
    int32_t measures;          /* 12  i/o  += 1 per measuring call */
    int32_t first_nonfinite_g; /* 16  out  the lowest row index with g_nonfinite != 0 at the last measuring call, -1 if none */
    int32_t first_nonfinite_p; /* 20  out  ... with p_nonfinite != 0 */
    int32_t reserved[10];      /* 24       not touched */
} frcnn_tensor_stats_state;
#define FRCNN_TENSOR_STATS_FINISH_THREADS 256
/* frcnn_tensor_stats: three launches whatever the tensors are, no host synchronisation, capturable, no atomics, no workgroup waits on
 * another, plain stores only.  It does not read the optimizer's skip word: the step that is skipped is the one whose culprit is wanted.
 *   partial  one workgroup of 256 threads per map entry.  It reads the chunk's g and p and, only if born[tensor] != 0, its m, and stores per
 *            chunk: three binary64 sums of squares, each by exactly the chunk contract of frcnn_grad_norm above (element, chunk, wave,
 *            block -- the same code, so the g partials are the bits frcnn_grad_norm leaves in its workspace; 0 for an unread m), max|g|
 *            and max|p| (binary32), the int32 non-finite counts of g and p.  Each stream takes 16-byte loads when ITS pointer is 16-byte
 *            aligned, dword loads otherwise; the element-to-thread assignment is the same.
 *   finish   one workgroup of T = FRCNN_TENSOR_STATS_FINISH_THREADS threads per tensor over that tensor's k chunk partials, in chunk
 *            order: thread t starts at +0 and adds partials t, t + T, t + 2T, ... in that order; then the xor butterfly inside each of
 *            the 4 waves; then ((w0 + w1) + w2) + w3 -- for each of the three sums.  Counts: the same tree in int64, saturated to
 *            INT32_MAX.  Maxima by max.  k == 0 (a tensor without elements): a row of zeros.  born[tensor] == 0: m_sumsq = +0, m_read = 0.
 *   advance  one workgroup.  On a measuring call it reads the rows: measured_tick = tick, measures += 1, first_nonfinite_g / _p as above.
 *            On every call tick = (tick + 1) & INT32_MAX.
 * Decimation on the device: partial and finish read tick and every first and return before any other load when tick % every != 0;
 * advance still moves tick.  A captured step therefore measures every Nth replay with one graph; rows, measured_tick and first_nonfinite_*
 * keep the last measured values in between.  A state block that is not ours (every < 1 or tick < 0), a map entry outside the table, a tensor
 * whose chunks are not where the map's order puts them: every kernel touches nothing.
 * Finite values cannot overflow a sum (see frcnn_grad_norm).  tests/tensor_stats_ref.py restates all of it in numpy.
 *
 * frcnn_tensor_stats_workspace_bytes(n_tensors, n_chunks): bytes for the partials,
 *   double g[n_chunks] | double p[n_chunks] | double m[n_chunks] | float gmax[n_chunks] | float pmax[n_chunks] | int32 gbad[n_chunks] |
 *   int32 pbad[n_chunks]
 * (at least 16); 0 for n_tensors outside 1 .. 65536 or a negative n_chunks.  16-byte aligned device memory, fully rewritten by a measuring
 * call, not touched by any other.  FRCNN_ERR_INVALID_ARG before anything is launched: a NULL table / born / rows / state / workspace,
 * n_tensors outside 1 .. 65536, a negative n_chunks, a table, rows, state or workspace that is not 16-byte aligned, a born that is not
 * 4-byte aligned, rows, state and workspace that overlap one another; FRCNN_ERR_WORKSPACE: a table shorter than n_tensors and n_chunks
 * need, a workspace shorter than frcnn_tensor_stats_workspace_bytes(n_tensors, n_chunks). */
size_t frcnn_tensor_stats_workspace_bytes(int n_tensors, int n_chunks);
int frcnn_tensor_stats(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const int32_t *born, frcnn_tensor_stats_row *rows,
                       frcnn_tensor_stats_state *state, void *workspace, size_t workspace_bytes, void *stream);

/* The journal: ring[capacity][n_cols] binary64, marks[capacity] int32, totals[n_cols], one state block, all DEVICE memory.  The caller
 * writes capacity and n_cols into the state block, zeroes the rest, and initialises every column's totals to
 * {sum +0, count 0, max -inf, min +inf, nonfinite 0}, outside any graph. */
typedef struct {
    double sum;              /*  0  i/o  the sequential binary64 sum of the column's FINITE values, in append order, one rounding per append */
    int64_t count;           /*  8  i/o  finite values appended */
    double max;              /* 16  i/o  the largest finite value (`>` comparison); the caller's -inf before the first */
    double min;              /* 24  i/o  the smallest finite value (`<` comparison); the caller's +inf before the first */
    int64_t nonfinite;       /* 32  i/o  inf and NaN values appended: in the ring as they are, in none of sum, max, min */
} frcnn_journal_totals;
typedef struct {
    int64_t cursor;          /*  0  i/o  appends so far; the next row goes to ring[cursor % capacity] */
    int32_t capacity;        /*  8  in   must equal the capacity argument */
    int32_t n_cols;          /* 12  in   must equal the n_cols argument */
    int32_t reserved[12];    /* 16       not touched */
} frcnn_journal_state;
#define FRCNN_JOURNAL_MAX_COLS 64
#define FRCNN_JOURNAL_F32 0
#define FRCNN_JOURNAL_F64 1
#define FRCNN_JOURNAL_I32 2
#define FRCNN_JOURNAL_I64 3
/* frcnn_journal_append: one launch of one wave, no host synchronisation, capturable, no atomics.  src_host / dtype_host are HOST arrays
 * of n_cols device pointers and FRCNN_JOURNAL_* codes; the library hands them to its kernel BY VALUE in the kernel arguments, which a
 * graph node stores (a loss tensor's address exists only inside the capture's pool).  Lane c < n_cols reads cursor and its source, widens
 * the value to binary64 (fp32, int32: exact; int64: round to nearest even), stores ring[cursor % capacity][c], and updates totals[c]:
 * finite: sum = sum + v (one rounding), count += 1, max, min; otherwise nonfinite += 1.  Behind a barrier lane 0 stores
 * marks[cursor % capacity] = mark ? *mark : 0 and cursor + 1.  Appends on one stream are ordered, so sum is the sequential binary64 sum in
 * append order: for a column of fp32 values the bits of SmoothedValue.total (util/misc.py:40-43, fed with loss.item(), the widened fp32),
 * and sum / count those of its global_avg.  A state block that is not ours (capacity or n_cols differ from the arguments, a negative
 * cursor): nothing is touched.  tests/journal_ref.py restates it.
 * FRCNN_ERR_INVALID_ARG before anything is launched: n_cols outside 1 .. 64; capacity < 1; a NULL array, source, ring, marks, totals or
 * state; a dtype code outside 0 .. 3; a source not aligned to its type; ring or totals not 8-byte aligned, marks or mark not 4-byte
 * aligned, state not 16-byte aligned; a source (or mark) that overlaps ring, marks, totals or state. */
int frcnn_journal_append(int n_cols, const void *const *src_host, const int32_t *dtype_host, int capacity, double *ring, int32_t *marks,
                         frcnn_journal_totals *totals, frcnn_journal_state *state, const int32_t *mark, void *stream);

/* ---- in-library kernel timing (HIP events on the launch stream) -------------------------------------- */
/* When enabled, every kernel launch made by this library is bracketed by two hipEventRecord on the
 * caller's stream.  frcnn_prof_collect() synchronises those events (call it after the stream is idle)
 * and folds them into per-kernel totals readable with frcnn_prof_get().                                 */
int frcnn_prof_enable(int on);
int frcnn_prof_collect(void);
int frcnn_prof_reset(void);
int frcnn_prof_num_kernels(void);
const char *frcnn_prof_kernel_name(int kernel_id);
int frcnn_prof_get(int kernel_id, double *total_ms, int64_t *launches);
/* per-launch durations (ms, launch order) of one kernel since the last reset: copies min(cap, n), returns n. */
int64_t frcnn_prof_get_samples(int kernel_id, float *out_ms, int64_t cap);

/* Diagnostics: n_workgroups workgroups of 256 threads that do nothing but stay resident for `microseconds` (bounded: <= 100 000) on
 * `stream` -- a stand-in for another tenant's persistent kernels (RCCL's channels during the gradient all-reduce) when testing that the
 * launches with in-kernel hand-offs (nms_kernel, rpn_match_kernel, topk_partition_kernel) still complete and stay exact next to them
 * (tests/test_gpu_ops.py: test_in_kernel_handoffs_next_to_resident_foreign_workgroups).  Not used by the product path.            */
int frcnn_diag_occupy(int n_workgroups, int microseconds, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FRCNN_HIP_H */
