// ema.hip -- an exponential moving average of the weights, kept in device memory.  The reference evaluates and checkpoints the raw
// weights (train.py:75-85) and has no average; detection trainers evaluate the averaged ones, and with one frame per step the raw ones are
// noisy.  Defined by this project, pinned to torch: per element, p the parameter after this update, e its average, w the float32 weight,
//   d  = round(p - e)
//   e' = |w| < 0.5 ? fma(w, d, e) : fma(round(w - 1), d, p)
// the bits of torch._foreach_lerp_([e], [p], w) on the CPU (torch.optim.swa_utils.get_ema_multi_avg_fn).  The library is built with
// -ffp-contract=off; every fused operation is written out (__fmaf_rn, ema_dev.h).
//
//   table   built on the host (frcnn_ema_table_build_host), uploaded by the caller:
//             EmaHeader | EmaRow[n_tensors] {parameter, shadow, numel, vec} | int2 map[n_chunks] {tensor, chunk in tensor}
//           chunked like the SGD table (sgd_dev.h): one workgroup per map entry, no search.
//   state   frcnn_ema_state (include/frcnn_hip.h), 64 bytes: decay, num_updates, w, flags, swapped, skipped, refused.  The update and the
//           fused step (sgd.hip) only READ it; ema_advance_kernel, one thread on the same stream behind them, computes the next w in
//           binary64 -- decay_t = warm-up ? min(decay, (1 + n) / (10 + n)) : decay, w = (float)(1 - decay_t) -- so no float is divided in
//           the update kernel and a captured graph follows the warm-up.  ema_swap_kernel's first thread toggles swapped.
//   skip    NULL, or a device int32: non-zero leaves the average and num_updates as they are (counted in skipped).  While swapped is set the
//           parameters HOLD the average: an update then changes nothing either (counted in refused).
//
// Memory: the update reads 8 B and writes 4 B per element, the swap reads 8 B and writes 8 B, nothing reused: streaming kernels.  16-byte
// accesses when both pointers of a row are 16-byte aligned (SGD_CHUNK is a multiple of 4, so every chunk of such a row starts aligned),
// four independent float4 pairs in flight per thread.  Any other row -- a view at an odd storage offset -- takes the dword path for its
// whole length: its two pointers need not share a misalignment.  No atomics, no LDS, no workgroup waits on another.
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
#include "ema_dev.h"
#include "multi_tensor_dev.h"
FRCNN_LAYOUT_STAMP(ema);

template <class T> struct EmaRegs { T p, e; };      // one index of a sweep (multi_tensor_dev.h): T is sgd_f4 or float

__global__ __launch_bounds__(SGD_THREADS) void ema_update_kernel(const EmaRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors,
                                                                 const frcnn_ema_state *__restrict__ st, const int32_t *__restrict__ skip)
{
    if (skip && *skip != 0) return;
    if (st->swapped != 0) return;
    const float w = st->w, wm1 = __fsub_rn(w, 1.0f);
    const bool small = fabsf(w) < 0.5f;
    MtChunk<EmaRow> c;
    if (!mt_chunk(rows, map, n_tensors, &c)) return;                        // a table that is not ours: touch nothing
    const float *p = c.row.p + c.off;
    float *e = c.row.e + c.off;
    const sgd_f4 *p4 = (const sgd_f4 *)p;
    sgd_f4 *e4 = (sgd_f4 *)e;
    mt_chunk_sweep<EmaRegs<sgd_f4>, EmaRegs<float>>(
        c.n, c.row.vec != 0,
        [&](EmaRegs<sgd_f4> &r, int i) {
            r.p = p4[i];
            r.e = e4[i];
        },
        [&](EmaRegs<sgd_f4> &r, int i) {
            sgd_f4 q;
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = ema_one(r.p[j], r.e[j], w, wm1, small);
            e4[i] = q;
        },
        [&](EmaRegs<float> &r, int i) {                                     // the tail of an aligned row; all of a misaligned one
            r.p = p[i];
            r.e = e[i];
        },
        [&](EmaRegs<float> &r, int i) { e[i] = ema_one(r.p, r.e, w, wm1, small); });
}

// p <-> e, element for element.  Not gated: the way back must always be open.  Workgroup 0's first thread toggles the swapped word; no
// workgroup of this launch reads it.  The grid has at least one workgroup, so the word moves even when every tensor is empty.
__global__ __launch_bounds__(SGD_THREADS) void ema_swap_kernel(const EmaRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors, int n_chunks,
                                                               frcnn_ema_state *__restrict__ st)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) st->swapped = st->swapped == 0;
    if ((int)blockIdx.x >= n_chunks) return;
    MtChunk<EmaRow> c;
    if (!mt_chunk(rows, map, n_tensors, &c)) return;                        // a table that is not ours: touch nothing
    float *p = c.row.p + c.off, *e = c.row.e + c.off;
    sgd_f4 *p4 = (sgd_f4 *)p, *e4 = (sgd_f4 *)e;
    mt_chunk_sweep<EmaRegs<sgd_f4>, EmaRegs<float>>(
        c.n, c.row.vec != 0,
        [&](EmaRegs<sgd_f4> &r, int i) {
            r.p = p4[i];
            r.e = e4[i];
        },
        [&](EmaRegs<sgd_f4> &r, int i) {
            p4[i] = r.e;
            e4[i] = r.p;
        },
        [&](EmaRegs<float> &r, int i) {
            r.p = p[i];
            r.e = e[i];
        },
        [&](EmaRegs<float> &r, int i) {
            p[i] = r.e;
            e[i] = r.p;
        });
}

// behind an update, one thread, the only writer of these words.  The next weight in binary64, as the host computes it for n = 0.
__global__ __launch_bounds__(WAVE) void ema_advance_kernel(frcnn_ema_state *__restrict__ st, const int32_t *__restrict__ skip)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (st->swapped != 0) {
        st->refused = st->refused + 1;
        return;
    }
    if (skip && *skip != 0) {
        st->skipped = st->skipped + 1;
        return;
    }
    const int64_t n = st->num_updates + 1;
    const double decay = st->decay;
    double dt = decay;
    if (st->flags & FRCNN_EMA_WARMUP) {
        const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
        if (ramp < decay) dt = ramp;                                        // Python's min(decay, ramp)
    }
    st->num_updates = n;
    st->w = (float)(1.0 - dt);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// Bytes of the table for these tensor sizes; 0 for what the builder refuses.
FRCNN_EXPORT size_t frcnn_ema_table_bytes(int n_tensors, const int64_t *numel_host)
{
    if (n_tensors < 1 || n_tensors > SGD_MAX_TENSORS || !numel_host) return 0;
    const int64_t chunks = mt_table_chunks(n_tensors, numel_host);
    return chunks < 0 ? 0 : ema_table_bytes(n_tensors, chunks);
}

// Fills the caller's HOST buffer; the caller uploads table_bytes bytes to 16-byte aligned device memory.
FRCNN_EXPORT int frcnn_ema_table_build_host(int n_tensors, const void *const *params_host, const void *const *shadows_host, const int64_t *numel_host,
                                            void *table_host, size_t table_bytes, int32_t *n_chunks_host)
{
    FRCNN_REQUIRE(params_host && shadows_host && numel_host && table_host && n_chunks_host, "ema_table_build: NULL argument");
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS, "ema_table_build: n_tensors %d outside 1 .. %d", n_tensors, SGD_MAX_TENSORS);
    const int rc = mt_check_rows("ema_table_build", n_tensors, numel_host, {params_host, shadows_host});
    if (rc != FRCNN_OK) return rc;
    const size_t need = frcnn_ema_table_bytes(n_tensors, numel_host);
    FRCNN_REQUIRE(need != 0, "ema_table_build: more than 2^31 - 1 chunks");
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "ema_table_build: short table, %zu < %zu bytes", table_bytes, need);
    // both are written (the shadow by the update, both by the swap): no two ranges may overlap, of one row or of two
    std::vector<Span> w;
    for (int t = 0; t < n_tensors; ++t) {
        mt_add_span(w, params_host[t], numel_host[t], t, 'p');
        mt_add_span(w, shadows_host[t], numel_host[t], t, 'e');
    }
    const MtOverlap o = mt_overlap(w, {});
    FRCNN_REQUIRE(o.what == 0, "ema_table_build: overlapping parameter and shadow (%c of row %d and %c of row %d)", o.a.kind, o.a.row, o.b.kind, o.b.row);
    const auto [rows, map] = mt_table<EmaHeader, EmaRow>(table_host, n_tensors);
    int64_t c = 0;
    for (int t = 0; t < n_tensors; ++t) {
        rows[t].p = (float *)params_host[t];
        rows[t].e = (float *)shadows_host[t];
        rows[t].numel = numel_host[t];
        rows[t].vec = (((uintptr_t)params_host[t] | (uintptr_t)shadows_host[t]) & 15) == 0;
        rows[t].pad = 0;
        const int64_t k = mt_chunks_of(numel_host[t]);
        for (int64_t j = 0; j < k; ++j) map[c++] = make_int2(t, (int)j);
    }
    *(EmaHeader *)table_host = EmaHeader{EMA_MAGIC, n_tensors, (int32_t)c, SGD_CHUNK, {0, 0, 0, 0}, sizeof(EmaHeader), sizeof(EmaHeader) + (size_t)n_tensors * sizeof(EmaRow), need, 0};
    *n_chunks_host = (int32_t)c;
    return FRCNN_OK;
}

static int ema_check(const char *who, const void *table, size_t table_bytes, int n_tensors, int n_chunks, const frcnn_ema_state *state, const int32_t *skip)
{
    FRCNN_REQUIRE(table && state, "%s: NULL pointer", who);
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS && n_chunks >= 0, "%s: bad counts (%d tensors, %d chunks)", who, n_tensors, n_chunks);
    FRCNN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)skip & 3) == 0,
                  "%s: table and state must be 16-byte aligned, skip 4-byte aligned", who);
    const size_t need = ema_table_bytes(n_tensors, n_chunks);
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "%s: short table, %zu < %zu bytes", who, table_bytes, need);
    return FRCNN_OK;
}

int ema_advance_launch(frcnn_ema_state *state, const int32_t *skip, hipStream_t stream)
{
    FRCNN_LAUNCH(ema_advance_kernel, dim3(1), dim3(WAVE), 0, stream, state, skip);
    FRCNN_CHECK_LAUNCH("ema_advance_kernel");
    return FRCNN_OK;
}

// The average behind any optimizer's step.  Two launches, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_ema_update(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_ema_state *state, const int32_t *skip, void *stream)
{
    const int rc = ema_check("ema_update", table, table_bytes, n_tensors, n_chunks, state, skip);
    if (rc != FRCNN_OK) return rc;
    const auto [rows, map] = mt_table<EmaHeader, EmaRow>(table, n_tensors);
    hipStream_t s = (hipStream_t)stream;
    if (n_chunks > 0)                                                       // every tensor empty: the bookkeeping alone
        FRCNN_LAUNCH(ema_update_kernel, dim3((unsigned)n_chunks), dim3(SGD_THREADS), 0, s, rows, map, n_tensors, (const frcnn_ema_state *)state, skip);
    return ema_advance_launch(state, skip, s);
}

// Live and averaged weights exchanged in place: one launch, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_ema_swap(const void *table, size_t table_bytes, int n_tensors, int n_chunks, frcnn_ema_state *state, void *stream)
{
    const int rc = ema_check("ema_swap", table, table_bytes, n_tensors, n_chunks, state, nullptr);
    if (rc != FRCNN_OK) return rc;
    const auto [rows, map] = mt_table<EmaHeader, EmaRow>(table, n_tensors);
    FRCNN_LAUNCH(ema_swap_kernel, dim3((unsigned)std::max(n_chunks, 1)), dim3(SGD_THREADS), 0, (hipStream_t)stream, rows, map, n_tensors, n_chunks, state);
    FRCNN_CHECK_LAUNCH("ema_swap_kernel");
    return FRCNN_OK;
}
