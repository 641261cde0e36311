// sgd.hip -- the optimizer step of the reference (main.py:58-61: torch.optim.SGD(lr, momentum, weight_decay), stepped at train.py:35-37)
// as ONE multi-tensor launch whose hyper-parameters are device data, so that a captured graph follows the learning-rate schedule.
//
//   table   built on the host (frcnn_sgd_table_build_host), uploaded by the caller:
//             SgdHeader | SgdRow[n_tensors] {parameter, gradient, momentum, numel, group, vec} | int2 map[n_chunks] {tensor, chunk in tensor}
//           One workgroup per map entry: SGD_CHUNK elements of one tensor.  No search: the block reads its own entry and its tensor's row.
//   hyper   float[G][4] = (lr, momentum, weight_decay, unused), read by every block at run time.
//   born    int32[n_tensors]: 0 until a tensor's momentum has been written once.  The update kernel only READS it; sgd_born_kernel, the
//           second launch on the same stream, sets the words after every block of the first has finished.
//   skip    NULL, or a device int32: non-zero turns both launches into no-ops.
//
// The rule, operation for operation (torch.optim.SGD, dampening 0, no Nesterov, maximize=False; the fused operations are torch's
// `add(x, alpha=a)`, one rounding):
//   d  = wd != 0 ? fma(wd, p, g) : g              no product with a zero weight decay: an infinite p stays infinite
//   m' = (first update or mu == 0) ? d : round(mu * m) + d
//   p' = fma(-lr, m', p)
// With mu == 0 torch keeps no momentum buffer: m is neither read nor written and the born word stays as it is.
// The library is built with -ffp-contract=off; every fused operation below is written out (__fmaf_rn).
//
// Memory: 12 B read + 8 B written per element, nothing reused: a streaming kernel.  16-byte accesses when a tensor's three pointers are
// 16-byte aligned (SGD_CHUNK is a multiple of 4, so every chunk of such a tensor starts aligned), four independent float4 triples in flight
// per thread; the gradient is read once and loaded non-temporally.  Any other tensor (a view at an odd storage offset) takes the
// dword path for its whole length, four dwords per array in flight.  The chunk lookup and the sweep are multi_tensor_dev.h's.
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
#include "sgd_dev.h"
#include "ema_dev.h"
#include "multi_tensor_dev.h"
FRCNN_LAYOUT_STAMP(sgd);

__device__ __forceinline__ float sgd_one(float p, float g, float *m, float neg_lr, float mu, float wd, bool use_wd, bool keep, bool first)
{
    const float d = use_wd ? __fmaf_rn(wd, p, g) : g;
    float mn = d;
    if (keep) {
        if (!first) mn = __fadd_rn(__fmul_rn(mu, *m), d);
        *m = mn;
    }
    return __fmaf_rn(neg_lr, mn, p);
}

// one index of a sweep (multi_tensor_dev.h): T is sgd_f4 or float.  m and e are loaded only where the rule reads them.
template <class T> struct SgdRegs { T p, g, m = T(0.0f), e = T(0.0f); };

// SCALE = false: the rule above on the gradient as it is.  SCALE = true: every gradient element is first multiplied by the device float
// *grad_scale (one rounding, __fmul_rn) -- the bits of torch's in-place g.mul_(coef) followed by torch.optim.SGD; the gradient itself is
// not written.
// EMA = true: the weight average (ema.hip, ema_dev.h) rides in the same pass: behind p' the kernel loads the shadow e, applies ema_one and
// stores e' -- p' is still in registers, so the average costs 8 B per element instead of a 12 B pass of its own.  The EMA row of a tensor
// stands under the same tensor number (the two maps are equal entry for entry); the shadow pointer is NOT covered by SgdRow.vec, so a row
// takes the 16-byte path only when both rows say so.  While the state's swapped word is set the parameters hold the average: the whole
// step changes nothing.  With EMA = false none of this is compiled in: the two instantiations of before are what they were.
template <bool SCALE, bool EMA>
__global__ __launch_bounds__(SGD_THREADS) void sgd_update_kernel(const SgdRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors,
                                                                 const float4 *__restrict__ hyper, int n_groups,
                                                                 const int32_t *__restrict__ born, const int32_t *__restrict__ skip,
                                                                 const float *__restrict__ grad_scale, const EmaRow *__restrict__ erows,
                                                                 const frcnn_ema_state *__restrict__ est)
{
    if (skip && *skip != 0) return;
    float w = 0.0f, wm1 = 0.0f;
    bool small = false;
    if (EMA) {
        if (est->swapped != 0) return;
        w = est->w;
        wm1 = __fsub_rn(w, 1.0f);
        small = fabsf(w) < 0.5f;
    }
    float gs = 1.0f;
    if (SCALE) gs = *grad_scale;
    MtChunk<SgdRow> c;
    if (!mt_chunk(rows, map, n_tensors, &c)) return;                        // a table that is not ours: touch nothing
    const SgdRow &r = c.row;
    if ((unsigned)r.group >= (unsigned)n_groups) return;
    const float4 h = hyper[r.group];
    const float neg_lr = -h.x, mu = h.y, wd = h.z;
    const bool use_wd = wd != 0.0f, keep = mu != 0.0f, first = born[c.tensor] == 0;
    float *p = r.p + c.off, *m = r.m + c.off;
    const float *g = r.g + c.off;
    float *e = nullptr;
    bool vec = r.vec != 0;
    if (EMA) {
        const EmaRow er = erows[c.tensor];
        if (er.p != r.p || er.numel != r.numel) return;                    // an EMA table that is not this table's: touch nothing
        e = er.e + c.off;
        vec = vec && er.vec != 0;
    }
    sgd_f4 *p4 = (sgd_f4 *)p, *m4 = (sgd_f4 *)m, *e4 = (sgd_f4 *)e;
    const sgd_f4 *g4 = (const sgd_f4 *)g;
    mt_chunk_sweep<SgdRegs<sgd_f4>, SgdRegs<float>>(
        c.n, vec,
        [&](SgdRegs<sgd_f4> &v, int i) {
            v.p = p4[i];
            v.g = __builtin_nontemporal_load(&g4[i]);
            if (keep && !first) v.m = m4[i];
            if (EMA) v.e = e4[i];
        },
        [&](SgdRegs<sgd_f4> &v, int i) {
            sgd_f4 q;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mj = v.m[j];
                q[j] = sgd_one(v.p[j], SCALE ? __fmul_rn(v.g[j], gs) : v.g[j], &mj, neg_lr, mu, wd, use_wd, keep, first);
                v.m[j] = mj;
            }
            if (keep) m4[i] = v.m;
            p4[i] = q;
            if (EMA) {
                sgd_f4 a;
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = ema_one(q[j], v.e[j], w, wm1, small);
                e4[i] = a;
            }
        },
        [&](SgdRegs<float> &v, int i) {                                     // the tail of an aligned tensor; all of a misaligned one
            v.p = p[i];
            v.g = g[i];
            if (keep && !first) v.m = m[i];
            if (EMA) v.e = e[i];
        },
        [&](SgdRegs<float> &v, int i) {
            const float q = sgd_one(v.p, SCALE ? __fmul_rn(v.g, gs) : v.g, &v.m, neg_lr, mu, wd, use_wd, keep, first);
            if (keep) m[i] = v.m;
            p[i] = q;
            if (EMA) e[i] = ema_one(q, v.e, w, wm1, small);
        });
}

// after the update: a tensor whose group keeps momentum has one now
// (est: NULL, or the state of the weight average fused into the update: while its swapped word is set the step did not happen)
__global__ __launch_bounds__(SGD_THREADS) void sgd_born_kernel(const SgdRow *__restrict__ rows, int n_tensors, const float4 *__restrict__ hyper, int n_groups,
                                                               int32_t *__restrict__ born, const int32_t *__restrict__ skip,
                                                               const frcnn_ema_state *__restrict__ est)
{
    if (skip && *skip != 0) return;
    if (est && est->swapped != 0) return;
    const int t = blockIdx.x * SGD_THREADS + threadIdx.x;
    if (t >= n_tensors) return;
    const int grp = rows[t].group;
    if ((unsigned)grp >= (unsigned)n_groups) return;
    if (hyper[grp].y != 0.0f) born[t] = 1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// main.py:58-61 / train.py:35-37.  Bytes of the table for these tensor sizes; 0 for what the builder refuses.
FRCNN_EXPORT size_t frcnn_sgd_table_bytes(int n_tensors, const int64_t *numel_host)
{
    if (n_tensors < 1 || n_tensors > SGD_MAX_TENSORS || !numel_host) return 0;
    const int64_t chunks = mt_table_chunks(n_tensors, numel_host);
    return chunks < 0 ? 0 : sgd_table_bytes(n_tensors, chunks);
}

// main.py:58-61 / train.py:35-37.  Fills the caller's HOST buffer; the caller uploads table_bytes bytes to 16-byte aligned device memory.
FRCNN_EXPORT int frcnn_sgd_table_build_host(int n_tensors, const void *const *params_host, const void *const *grads_host, const void *const *moms_host,
                                            const int64_t *numel_host, const int32_t *group_host, int n_groups, void *table_host, size_t table_bytes,
                                            int32_t *n_chunks_host)
{
    FRCNN_REQUIRE(params_host && grads_host && moms_host && numel_host && group_host && table_host && n_chunks_host, "sgd_table_build: NULL argument");
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS, "sgd_table_build: n_tensors %d outside 1 .. %d", n_tensors, SGD_MAX_TENSORS);
    FRCNN_REQUIRE(n_groups >= 1 && n_groups <= SGD_MAX_GROUPS, "sgd_table_build: n_groups %d outside 1 .. %d", n_groups, SGD_MAX_GROUPS);
    const int rc = mt_check_rows("sgd_table_build", n_tensors, numel_host, {params_host, grads_host, moms_host});
    if (rc != FRCNN_OK) return rc;
    for (int t = 0; t < n_tensors; ++t)
        FRCNN_REQUIRE(group_host[t] >= 0 && group_host[t] < n_groups, "sgd_table_build: row %d names group %d outside 0 .. %d", t, group_host[t], n_groups - 1);
    const size_t need = frcnn_sgd_table_bytes(n_tensors, numel_host);
    FRCNN_REQUIRE(need != 0, "sgd_table_build: more than 2^31 - 1 chunks");
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "sgd_table_build: short table, %zu < %zu bytes", table_bytes, need);
    // written: parameter and momentum ranges (all rows); read only: the gradients
    std::vector<Span> w, ro;
    for (int t = 0; t < n_tensors; ++t) {
        mt_add_span(w, params_host[t], numel_host[t], t, 'p');
        mt_add_span(w, moms_host[t], numel_host[t], t, 'm');
        mt_add_span(ro, grads_host[t], numel_host[t], t, 'g');
    }
    const MtOverlap o = mt_overlap(w, ro);
    FRCNN_REQUIRE(o.what != 1, "sgd_table_build: overlapping parameter and momentum (%c of row %d and %c of row %d)", o.a.kind, o.a.row, o.b.kind, o.b.row);
    FRCNN_REQUIRE(o.what != 2, "sgd_table_build: the gradient of row %d overlaps a parameter or a momentum", o.a.row);
    const auto [rows, map] = mt_table<SgdHeader, SgdRow>(table_host, n_tensors);
    int64_t c = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const uintptr_t all = (uintptr_t)params_host[t] | (uintptr_t)grads_host[t] | (uintptr_t)moms_host[t];
        rows[t].p = (float *)params_host[t];
        rows[t].g = (const float *)grads_host[t];
        rows[t].m = (float *)moms_host[t];
        rows[t].numel = numel_host[t];
        rows[t].group = group_host[t];
        rows[t].vec = (all & 15) == 0;
        rows[t].pad[0] = rows[t].pad[1] = 0;
        const int64_t k = mt_chunks_of(numel_host[t]);
        for (int64_t j = 0; j < k; ++j) map[c++] = make_int2(t, (int)j);
    }
    *(SgdHeader *)table_host = SgdHeader{SGD_MAGIC, n_tensors, n_groups, (int32_t)c, SGD_CHUNK, {0, 0, 0}, sizeof(SgdHeader),
                      sizeof(SgdHeader) + (size_t)n_tensors * sizeof(SgdRow), need, 0};
    *n_chunks_host = (int32_t)c;
    return FRCNN_OK;
}

static int sgd_step_launch(const char *who, const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                           const int32_t *skip, const float *grad_scale, bool scaled, const void *ema_table, size_t ema_bytes,
                           frcnn_ema_state *ema_state, bool ema, void *stream)
{
    FRCNN_REQUIRE(table && hyper && born && (!scaled || grad_scale) && (!ema || (ema_table && ema_state)), "%s: NULL pointer", who);
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS && n_chunks >= 0, "%s: bad counts (%d tensors, %d chunks)", who, n_tensors, n_chunks);
    FRCNN_REQUIRE(n_groups >= 1 && n_groups <= SGD_MAX_GROUPS, "%s: n_groups %d outside 1 .. %d", who, n_groups, SGD_MAX_GROUPS);
    FRCNN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)hyper & 15) == 0 && ((uintptr_t)born & 3) == 0 && ((uintptr_t)skip & 3) == 0 &&
                      ((uintptr_t)grad_scale & 3) == 0,
                  "%s: table and hyper must be 16-byte aligned, born, skip and grad_scale 4-byte aligned", who);
    FRCNN_REQUIRE(((uintptr_t)ema_table & 15) == 0 && ((uintptr_t)ema_state & 15) == 0, "%s: the EMA table and state must be 16-byte aligned", who);
    const size_t need = sgd_table_bytes(n_tensors, n_chunks);
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "%s: short table, %zu < %zu bytes", who, table_bytes, need);
    if (ema && ema_bytes < ema_table_bytes(n_tensors, n_chunks))
        return frcnn_set_error(FRCNN_ERR_WORKSPACE, "%s: short EMA table, %zu < %zu bytes", who, ema_bytes, ema_table_bytes(n_tensors, n_chunks));
    hipStream_t s = (hipStream_t)stream;
    if (n_chunks == 0) return ema ? ema_advance_launch(ema_state, skip, s) : FRCNN_OK;      // every tensor is empty
    const auto [rows, map] = mt_table<SgdHeader, SgdRow>(table, n_tensors);
    const EmaRow *erows = ema ? mt_table<EmaHeader, EmaRow>(ema_table, n_tensors).rows : nullptr;
    const frcnn_ema_state *est = ema ? ema_state : nullptr;
    const float *gs = scaled ? grad_scale : nullptr;
#define SGD_UPDATE(S, E)                                                                                                                            \
    FRCNN_LAUNCH((sgd_update_kernel<S, E>), dim3((unsigned)n_chunks), dim3(SGD_THREADS), 0, s, rows, map, n_tensors, (const float4 *)hyper, n_groups, \
                 (const int32_t *)born, skip, gs, erows, est)
    if (ema) {
        if (scaled) SGD_UPDATE(true, true);
        else SGD_UPDATE(false, true);
    } else {
        if (scaled) SGD_UPDATE(true, false);
        else SGD_UPDATE(false, false);
    }
#undef SGD_UPDATE
    FRCNN_LAUNCH(sgd_born_kernel, dim3((unsigned)((n_tensors + SGD_THREADS - 1) / SGD_THREADS)), dim3(SGD_THREADS), 0, s, rows, n_tensors,
                 (const float4 *)hyper, n_groups, born, skip, est);
    FRCNN_CHECK_LAUNCH("sgd kernels");
    return ema ? ema_advance_launch(ema_state, skip, s) : FRCNN_OK;
}

// train.py:35-37 (optimizer.step()) for the optimizer main.py:58-61 constructs.  Two launches, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_sgd_step(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                                const int32_t *skip, void *stream)
{
    return sgd_step_launch("sgd_step", table, table_bytes, n_tensors, n_chunks, hyper, n_groups, born, skip, nullptr, false, nullptr, 0, nullptr, false, stream);
}

// train.py:35-37 with the gradient clipping torch.nn.utils.clip_grad_norm_ would do in front of optimizer.step(): the same two launches,
// every gradient element multiplied by the device float *grad_scale (frcnn_grad_norm's coef) on its way into the rule.
FRCNN_EXPORT int frcnn_sgd_step_scaled(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                                       const int32_t *skip, const float *grad_scale, void *stream)
{
    return sgd_step_launch("sgd_step_scaled", table, table_bytes, n_tensors, n_chunks, hyper, n_groups, born, skip, grad_scale, true, nullptr, 0, nullptr, false,
                           stream);
}

// train.py:35-37 with the weight average (ema.hip) fused into the update: either of the two above (grad_scale NULL or given), then the
// average's one-thread bookkeeping: three launches, one skip word for all of them, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_sgd_step_ema(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const float *hyper, int n_groups, int32_t *born,
                                    const int32_t *skip, const float *grad_scale, const void *ema_table, size_t ema_table_bytes, frcnn_ema_state *ema_state,
                                    void *stream)
{
    return sgd_step_launch("sgd_step_ema", table, table_bytes, n_tensors, n_chunks, hyper, n_groups, born, skip, grad_scale, grad_scale != nullptr, ema_table,
                           ema_table_bytes, ema_state, true, stream);
}
