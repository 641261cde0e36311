// grad_norm.hip -- what torch.nn.utils.clip_grad_norm_ computes in front of optimizer.step() (train.py:35-37), as device data: the global
// L2 norm of every gradient of an SGD table (sgd_dev.h; rows and chunk map reused as they are), the number of non-finite elements, and
// from them a clip coefficient and a skip word in a device state block (frcnn_grad_norm_state, include/frcnn_hip.h).  The update
// (sgd.hip, sgd_update_kernel<true>) multiplies the coefficient in; the gradients are read here and never written.
//
//   grad_norm_partial_kernel   one workgroup per map entry, as sgd_update_kernel: reads SGD_CHUNK gradient elements, 4 B per element, and
//                              stores one binary64 partial and one int32 count per chunk with plain stores.
//   grad_norm_finish_kernel    one workgroup: adds the partials and counts, writes the state block.
// No atomics, no workgroup waits on another: two launches, capturable, and the sum is the same bits on every run.
//
// The order of the additions is the contract written down in include/frcnn_hip.h (and restated in tests/grad_norm_ref.py): it depends on
// an element's position in its tensor only.  The square of a binary32 is exact in binary64, so fma(d, d, acc) and acc + d * d are the
// same number and contraction cannot change a bit; every other addition below is written out.  The chunk body (element, chunk, wave)
// lives in sumsq_dev.h, which telemetry.hip's per-tensor statistics run too.
//
// Loads: 16-byte when the chunk's GRADIENT pointer is 16-byte aligned (decided from g alone -- SgdRow.vec also covers p and m), dword
// loads otherwise, with the same element-to-thread assignment.  Default cache policy: the update reads the same bytes next.
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
#include "sgd_dev.h"
#include "multi_tensor_dev.h"
#include "sumsq_dev.h"
FRCNN_LAYOUT_STAMP(grad_norm);

#define GN_FINISH_THREADS FRCNN_GRAD_NORM_FINISH_THREADS
static_assert(GN_FINISH_THREADS % WAVE == 0 && GN_FINISH_THREADS <= 1024, "the finish kernel is one workgroup of whole waves");

__global__ __launch_bounds__(SGD_THREADS) void grad_norm_partial_kernel(const SgdRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors,
                                                                        double *__restrict__ partial, int32_t *__restrict__ bad_out)
{
    MtChunk<SgdRow> c = {};                                                 // a table that is not ours: c stays zeroed -- a zero partial, nothing read
    mt_chunk(rows, map, n_tensors, &c);
    const int tid = threadIdx.x;
    int bad;
    float unused;
    const double s = sumsq_chunk_wave<false>(c.row.g + c.off, c.n, tid, bad, unused);   // element, chunk, wave of the contract: sumsq_dev.h
    __shared__ double ws[SGD_THREADS / WAVE];
    __shared__ int wb[SGD_THREADS / WAVE];
    if ((tid & (WAVE - 1)) == 0) {
        ws[tid / WAVE] = s;
        wb[tid / WAVE] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        partial[blockIdx.x] = sumsq_block4(ws);
        bad_out[blockIdx.x] = wb[0] + wb[1] + wb[2] + wb[3];
    }
}

__global__ __launch_bounds__(GN_FINISH_THREADS) void grad_norm_finish_kernel(const double *__restrict__ partial, const int32_t *__restrict__ bad_in, int n_chunks,
                                                                             frcnn_grad_norm_state *__restrict__ st, const int32_t *__restrict__ user_guard)
{
    const int tid = threadIdx.x;
    double s = 0.0;
    long long bad = 0;
    for (int i = tid; i < n_chunks; i += GN_FINISH_THREADS) {
        s = __dadd_rn(s, partial[i]);
        bad += bad_in[i];
    }
    s = wave_sum_xor(s);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d, WAVE);
    __shared__ double ws[GN_FINISH_THREADS / WAVE];
    __shared__ long long wb[GN_FINISH_THREADS / WAVE];
    if ((tid & (WAVE - 1)) == 0) {
        ws[tid / WAVE] = s;
        wb[tid / WAVE] = bad;
    }
    __syncthreads();
    if (tid != 0) return;
    double sumsq = ws[0];
    long long nb = wb[0];
    for (int w = 1; w < GN_FINISH_THREADS / WAVE; ++w) {
        sumsq = __dadd_rn(sumsq, ws[w]);
        nb += wb[w];
    }
    const float norm = __double2float_rn(__dsqrt_rn(sumsq));
    const uint32_t flags = st->flags;
    float coef = 1.0f;
    if (flags & FRCNN_GRAD_NORM_CLIP) {
        const float c = __fdiv_rn(st->max_norm, __fadd_rn(norm, 1e-6f));
        coef = c > 1.0f ? 1.0f : c;                                         // a NaN stays a NaN, as torch.clamp leaves it
    }
    const int32_t nonfinite = nb > 0x7fffffffLL ? 0x7fffffff : (int32_t)nb;
    const int32_t skip = (((flags & FRCNN_GRAD_NORM_SKIP_NONFINITE) && nonfinite != 0) || (user_guard && *user_guard != 0)) ? 1 : 0;
    st->sumsq = sumsq;
    st->norm = norm;
    st->coef = coef;
    st->skip = skip;
    st->nonfinite = nonfinite;
    st->steps = st->steps + 1;
    st->skipped_steps = st->skipped_steps + skip;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// workspace: double partial[n_chunks] | int32 count[n_chunks]
FRCNN_EXPORT size_t frcnn_grad_norm_workspace_bytes(int n_chunks)
{
    if (n_chunks < 0) return 0;
    const size_t b = align_up((size_t)n_chunks * (sizeof(double) + sizeof(int32_t)), 16);
    return b < 16 ? 16 : b;
}

// train.py:35-37 (what clip_grad_norm_ measures in front of optimizer.step()).  Two launches, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_grad_norm(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_grad_norm_state *state, const int32_t *user_guard,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(table && state && workspace, "grad_norm: NULL pointer");
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS && n_chunks >= 0, "grad_norm: bad counts (%d tensors, %d chunks)", n_tensors, n_chunks);
    FRCNN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)user_guard & 3) == 0,
                  "grad_norm: table, state and workspace must be 16-byte aligned, user_guard 4-byte aligned");
    const size_t need = sgd_table_bytes(n_tensors, n_chunks);
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "grad_norm: short table, %zu < %zu bytes", table_bytes, need);
    const size_t ws_need = frcnn_grad_norm_workspace_bytes(n_chunks);
    if (workspace_bytes < ws_need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "grad_norm: short workspace, %zu < %zu bytes", workspace_bytes, ws_need);
    const auto [rows, map] = mt_table<SgdHeader, SgdRow>(table, n_tensors);
    double *partial = (double *)workspace;
    int32_t *bad = (int32_t *)((char *)workspace + (size_t)n_chunks * sizeof(double));
    hipStream_t s = (hipStream_t)stream;
    if (n_chunks > 0)
        FRCNN_LAUNCH(grad_norm_partial_kernel, dim3((unsigned)n_chunks), dim3(SGD_THREADS), 0, s, rows, map, n_tensors, partial, bad);
    FRCNN_LAUNCH(grad_norm_finish_kernel, dim3(1), dim3(GN_FINISH_THREADS), 0, s, (const double *)partial, (const int32_t *)bad, n_chunks, state, user_guard);
    FRCNN_CHECK_LAUNCH("grad_norm kernels");
    return FRCNN_OK;
}
