// telemetry.hip -- a record of a captured training run that costs no host synchronisation.  The reference prints its losses and the lr
// every vis_step steps from host floats (train.py:39-72, SmoothedValue util/misc.py:27-86: one loss.item() per step); a graph-replayed
// run keeps two things in device memory instead (structs, summation order and every refusal: include/frcnn_hip.h):
//
//   frcnn_tensor_stats     per-tensor statistics over an SGD table (sgd_dev.h; rows, chunk map and the born words reused as they are):
//     tensor_stats_partial_kernel   one workgroup per map entry, as grad_norm_partial_kernel: the chunk's g and p and, if the tensor is
//                                   born, its m: three binary64 sums of squares (sumsq_dev.h -- the code grad_norm.hip runs), max|g|, max|p|,
//                                   the non-finite counts of g and p, one plain store each per chunk.
//     tensor_stats_finish_kernel    one workgroup per tensor: adds that tensor's chunk partials in a fixed order, writes its 64-byte row.
//     tensor_stats_advance_kernel   one workgroup: the lowest row with a non-finite count, the tick bookkeeping.
//   Decimation is device data: partial and finish return before any other load unless tick % every == 0.
//
//   frcnn_journal_append   one row of up to 64 scalars into a ring, running totals per column.  One launch of one wave; the source
//                          pointers travel BY VALUE in the kernel arguments (JournalArgs, as grad_accum.hip's GaArgs): a loss tensor's
//                          address exists only inside the capture's pool, where no table can be uploaded.
//
// No atomics, no workgroup waits on another, plain stores only; gradients, parameters and momenta are never written.  A state block that
// is not ours makes every kernel touch nothing.  Memory: 12 B read per element of a born tensor (8 B unborn), nothing reused: a streaming
// pass bound by HBM.  The library is built with -ffp-contract=off; every binary64 addition is written out (__dadd_rn).
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
#include "sgd_dev.h"
#include "multi_tensor_dev.h"
#include "sumsq_dev.h"
FRCNN_LAYOUT_STAMP(telemetry);

#define TS_FINISH_THREADS FRCNN_TENSOR_STATS_FINISH_THREADS
#define TS_WAVES (TS_FINISH_THREADS / WAVE)
static_assert(TS_FINISH_THREADS == 4 * WAVE, "the finish kernel adds four waves in order");

// the workspace: double g | double p | double m | float gmax | float pmax | int32 gbad | int32 pbad, n_chunks of each
struct TsWork { double *g, *p, *m; float *gmax, *pmax; int32_t *gbad, *pbad; };

static inline TsWork ts_carve(void *workspace, int64_t n_chunks)
{
    TsWork w;
    w.g = (double *)workspace;
    w.p = w.g + n_chunks;
    w.m = w.p + n_chunks;
    w.gmax = (float *)(w.m + n_chunks);
    w.pmax = w.gmax + n_chunks;
    w.gbad = (int32_t *)(w.pmax + n_chunks);
    w.pbad = w.gbad + n_chunks;
    return w;
}

__device__ __forceinline__ bool ts_measures(const frcnn_tensor_stats_state *st)
{
    const int every = st->every, tick = st->tick;
    return every >= 1 && tick >= 0 && tick % every == 0;                    // a state that is not ours measures nothing
}

__global__ __launch_bounds__(SGD_THREADS) void tensor_stats_partial_kernel(const SgdRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors,
                                                                           const int32_t *__restrict__ born, const frcnn_tensor_stats_state *__restrict__ st,
                                                                           const TsWork w)
{
    if (!ts_measures(st)) return;                                           // before any other load
    MtChunk<SgdRow> c = {};                                                 // a table that is not ours: c stays zeroed -- zero partials, nothing read
    mt_chunk(rows, map, n_tensors, &c);
    const int n = c.n;
    const float *g = c.row.g + c.off, *p = c.row.p + c.off;
    const float *m = (n != 0 && born[c.tensor] != 0) ? c.row.m + c.off : nullptr;      // an unborn momentum is never loaded
    const int tid = threadIdx.x;
    int gbad, pbad, unused_bad;
    float gmax, pmax, unused_max;
    const double gs = sumsq_chunk_wave<true>(g, n, tid, gbad, gmax);
    const double ps = sumsq_chunk_wave<true>(p, n, tid, pbad, pmax);
    const double ms = sumsq_chunk_wave<false>(m, m ? n : 0, tid, unused_bad, unused_max);
    __shared__ double ws[3][SGD_THREADS / WAVE];
    __shared__ float wm[2][SGD_THREADS / WAVE];
    __shared__ int wb[2][SGD_THREADS / WAVE];
    if ((tid & (WAVE - 1)) == 0) {
        const int v = tid / WAVE;
        ws[0][v] = gs, ws[1][v] = ps, ws[2][v] = ms;
        wm[0][v] = gmax, wm[1][v] = pmax;
        wb[0][v] = gbad, wb[1][v] = pbad;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned b = blockIdx.x;
        w.g[b] = sumsq_block4(ws[0]);
        w.p[b] = sumsq_block4(ws[1]);
        w.m[b] = sumsq_block4(ws[2]);
        w.gmax[b] = fmaxf(fmaxf(wm[0][0], wm[0][1]), fmaxf(wm[0][2], wm[0][3]));   // no NaN among them: order-free
        w.pmax[b] = fmaxf(fmaxf(wm[1][0], wm[1][1]), fmaxf(wm[1][2], wm[1][3]));
        w.gbad[b] = wb[0][0] + wb[0][1] + wb[0][2] + wb[0][3];
        w.pbad[b] = wb[1][0] + wb[1][1] + wb[1][2] + wb[1][3];
    }
}

__device__ __forceinline__ long long ts_wave_sum_i64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

__global__ __launch_bounds__(TS_FINISH_THREADS) void tensor_stats_finish_kernel(const SgdRow *__restrict__ rows, const int2 *__restrict__ map, int n_tensors,
                                                                                int n_chunks, const int32_t *__restrict__ born,
                                                                                const frcnn_tensor_stats_state *__restrict__ st, const TsWork w,
                                                                                frcnn_tensor_stats_row *__restrict__ out)
{
    if (!ts_measures(st)) return;                                           // before any other load
    const int t = (int)blockIdx.x;
    if (t >= n_tensors) return;
    const int64_t numel = rows[t].numel;
    if (numel < 0) return;
    const int64_t k64 = mt_chunks_of(numel);
    int lo = 0, hi = n_chunks;                                              // the first map entry of a tensor >= t: uniform, scalar loads
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (map[mid].x < t) lo = mid + 1;
        else hi = mid;
    }
    if (k64 > (int64_t)(n_chunks - lo)) return;                             // a table that is not ours: touch nothing
    const int k = (int)k64, first = lo;
    if (k > 0) {
        const int2 a = map[first], z = map[first + k - 1];
        if (a.x != t || a.y != 0 || z.x != t || z.y != k - 1) return;
    }
    const int tid = threadIdx.x;
    const bool has_m = born[t] != 0;
    double s[3] = {0.0, 0.0, 0.0};
    long long gb = 0, pb = 0;
    float gm = 0.0f, pm = 0.0f;
    for (int i = tid; i < k; i += TS_FINISH_THREADS) {
        s[0] = __dadd_rn(s[0], w.g[first + i]);
        s[1] = __dadd_rn(s[1], w.p[first + i]);
        s[2] = __dadd_rn(s[2], w.m[first + i]);
        gm = fmaxf(gm, w.gmax[first + i]);
        pm = fmaxf(pm, w.pmax[first + i]);
        gb += w.gbad[first + i];
        pb += w.pbad[first + i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = wave_sum_xor(s[j]);
    gm = wave_max_xor(gm);
    pm = wave_max_xor(pm);
    gb = ts_wave_sum_i64(gb);
    pb = ts_wave_sum_i64(pb);
    __shared__ double ws[3][TS_WAVES];
    __shared__ float wm[2][TS_WAVES];
    __shared__ long long wb[2][TS_WAVES];
    if ((tid & (WAVE - 1)) == 0) {
        const int v = tid / WAVE;
        ws[0][v] = s[0], ws[1][v] = s[1], ws[2][v] = s[2];
        wm[0][v] = gm, wm[1][v] = pm;
        wb[0][v] = gb, wb[1][v] = pb;
    }
    __syncthreads();
    if (tid != 0) return;
    const long long gn = ((wb[0][0] + wb[0][1]) + wb[0][2]) + wb[0][3], pn = ((wb[1][0] + wb[1][1]) + wb[1][2]) + wb[1][3];
    frcnn_tensor_stats_row r;
    r.g_sumsq = sumsq_block4(ws[0]);
    r.p_sumsq = sumsq_block4(ws[1]);
    r.m_sumsq = has_m ? sumsq_block4(ws[2]) : 0.0;
    r.g_absmax = fmaxf(fmaxf(wm[0][0], wm[0][1]), fmaxf(wm[0][2], wm[0][3]));
    r.p_absmax = fmaxf(fmaxf(wm[1][0], wm[1][1]), fmaxf(wm[1][2], wm[1][3]));
    r.g_nonfinite = gn > 0x7fffffffLL ? 0x7fffffff : (int32_t)gn;
    r.p_nonfinite = pn > 0x7fffffffLL ? 0x7fffffff : (int32_t)pn;
    r.m_read = (has_m && k > 0) ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) r.reserved[j] = 0;
    out[t] = r;
}

__global__ __launch_bounds__(TS_FINISH_THREADS) void tensor_stats_advance_kernel(const frcnn_tensor_stats_row *__restrict__ rows, int n_tensors,
                                                                                 frcnn_tensor_stats_state *__restrict__ st)
{
    const int every = st->every, tick = st->tick;
    if (every < 1 || tick < 0) return;                                      // a state that is not ours: touch nothing
    const bool measured = tick % every == 0;
    const int tid = threadIdx.x;
    int fg = 0x7fffffff, fp = 0x7fffffff;
    if (measured) {
        for (int t = tid; t < n_tensors; t += TS_FINISH_THREADS) {          // increasing t: a thread's first hit is its lowest
            if (fg == 0x7fffffff && rows[t].g_nonfinite != 0) fg = t;
            if (fp == 0x7fffffff && rows[t].p_nonfinite != 0) fp = t;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            fg = min(fg, __shfl_xor(fg, d, WAVE));
            fp = min(fp, __shfl_xor(fp, d, WAVE));
        }
    }
    __shared__ int wf[2][TS_WAVES];
    if ((tid & (WAVE - 1)) == 0) {
        wf[0][tid / WAVE] = fg;
        wf[1][tid / WAVE] = fp;
    }
    __syncthreads();
    if (tid != 0) return;
    if (measured) {
        fg = min(min(wf[0][0], wf[0][1]), min(wf[0][2], wf[0][3]));
        fp = min(min(wf[1][0], wf[1][1]), min(wf[1][2], wf[1][3]));
        st->measured_tick = tick;
        st->measures = st->measures + 1;
        st->first_nonfinite_g = fg == 0x7fffffff ? -1 : fg;
        st->first_nonfinite_p = fp == 0x7fffffff ? -1 : fp;
    }
    st->tick = (int32_t)(((uint32_t)tick + 1u) & 0x7fffffffu);
}

// ---- the journal --------------------------------------------------------------------------------------------------------------------
#define JR_COLS FRCNN_JOURNAL_MAX_COLS
static_assert(JR_COLS == WAVE, "one lane per column");

struct JournalArgs {
    const void *src[JR_COLS];
    int8_t dtype[JR_COLS];
    int32_t n_cols, capacity;
};
static_assert(sizeof(JournalArgs) <= 1024, "JournalArgs and the other arguments must fit well inside the 4 KB kernel-argument segment");

__global__ __launch_bounds__(WAVE) void journal_append_kernel(const JournalArgs a, double *__restrict__ ring, int32_t *__restrict__ marks,
                                                              frcnn_journal_totals *__restrict__ totals, frcnn_journal_state *__restrict__ st,
                                                              const int32_t *__restrict__ mark)
{
    const int64_t cursor = st->cursor;
    if (st->capacity != a.capacity || st->n_cols != a.n_cols || cursor < 0) return;     // a state that is not ours: touch nothing
    if (a.n_cols < 1 || a.n_cols > JR_COLS || a.capacity < 1) return;
    const int slot = (int)(cursor % a.capacity);
    const int c = threadIdx.x;
    if (c < a.n_cols) {
        double v;
        switch (a.dtype[c]) {
        case FRCNN_JOURNAL_F32: v = (double)*(const float *)a.src[c]; break;
        case FRCNN_JOURNAL_F64: v = *(const double *)a.src[c]; break;
        case FRCNN_JOURNAL_I32: v = (double)*(const int32_t *)a.src[c]; break;
        default: v = __ll2double_rn(*(const long long *)a.src[c]); break;
        }
        ring[(size_t)slot * a.n_cols + c] = v;
        frcnn_journal_totals t = totals[c];
        if (((__double_as_longlong(v) >> 52) & 0x7ff) == 0x7ff) {
            t.nonfinite += 1;
        } else {
            t.sum = __dadd_rn(t.sum, v);
            t.count += 1;
            if (v > t.max) t.max = v;
            if (v < t.min) t.min = v;
        }
        totals[c] = t;
    }
    __syncthreads();                                                        // every lane has read the cursor
    if (c == 0) {
        marks[slot] = mark ? *mark : 0;
        st->cursor = cursor + 1;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
FRCNN_EXPORT size_t frcnn_tensor_stats_workspace_bytes(int n_tensors, int n_chunks)
{
    if (n_tensors < 1 || n_tensors > SGD_MAX_TENSORS || n_chunks < 0) return 0;
    const size_t b = align_up((size_t)n_chunks * (3 * sizeof(double) + 2 * sizeof(float) + 2 * sizeof(int32_t)), 16);
    return b < 16 ? 16 : b;
}

static inline bool tm_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    return na != 0 && nb != 0 && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// What a run reports in place of train.py:39-72's prints, per tensor.  Three launches, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_tensor_stats(const void *table, size_t table_bytes, int n_tensors, int n_chunks, const int32_t *born, frcnn_tensor_stats_row *rows,
                                    frcnn_tensor_stats_state *state, void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(table && born && rows && state && workspace, "tensor_stats: NULL pointer");
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS && n_chunks >= 0, "tensor_stats: bad counts (%d tensors, %d chunks)", n_tensors, n_chunks);
    FRCNN_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)rows & 15) == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                      ((uintptr_t)born & 3) == 0,
                  "tensor_stats: table, rows, state and workspace must be 16-byte aligned, born 4-byte aligned");
    const size_t need = sgd_table_bytes(n_tensors, n_chunks);
    if (table_bytes < need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "tensor_stats: short table, %zu < %zu bytes", table_bytes, need);
    const size_t ws_need = frcnn_tensor_stats_workspace_bytes(n_tensors, n_chunks);
    if (workspace_bytes < ws_need)
        return frcnn_set_error(FRCNN_ERR_WORKSPACE, "tensor_stats: short workspace, %zu < %zu bytes", workspace_bytes, ws_need);
    const size_t rows_bytes = (size_t)n_tensors * sizeof(frcnn_tensor_stats_row);
    FRCNN_REQUIRE(!tm_overlap(rows, rows_bytes, state, sizeof(*state)) && !tm_overlap(rows, rows_bytes, workspace, ws_need) &&
                      !tm_overlap(state, sizeof(*state), workspace, ws_need),
                  "tensor_stats: rows, state and workspace overlap");
    const auto [trows, map] = mt_table<SgdHeader, SgdRow>(table, n_tensors);
    const TsWork w = ts_carve(workspace, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    if (n_chunks > 0)
        FRCNN_LAUNCH(tensor_stats_partial_kernel, dim3((unsigned)n_chunks), dim3(SGD_THREADS), 0, s, trows, map, n_tensors, born,
                     (const frcnn_tensor_stats_state *)state, w);
    FRCNN_LAUNCH(tensor_stats_finish_kernel, dim3((unsigned)n_tensors), dim3(TS_FINISH_THREADS), 0, s, trows, map, n_tensors, n_chunks, born,
                 (const frcnn_tensor_stats_state *)state, w, rows);
    FRCNN_LAUNCH(tensor_stats_advance_kernel, dim3(1), dim3(TS_FINISH_THREADS), 0, s, (const frcnn_tensor_stats_row *)rows, n_tensors, state);
    FRCNN_CHECK_LAUNCH("tensor_stats kernels");
    return FRCNN_OK;
}

// What SmoothedValue.update (util/misc.py:40-43) keeps per printed quantity, for up to 64 of them at once.  One launch, capturable.
FRCNN_EXPORT int frcnn_journal_append(int n_cols, const void *const *src_host, const int32_t *dtype_host, int capacity, double *ring, int32_t *marks,
                                      frcnn_journal_totals *totals, frcnn_journal_state *state, const int32_t *mark, void *stream)
{
    FRCNN_REQUIRE(n_cols >= 1 && n_cols <= JR_COLS, "journal_append: n_cols %d outside 1 .. %d", n_cols, JR_COLS);
    FRCNN_REQUIRE(capacity >= 1, "journal_append: capacity %d < 1", capacity);
    FRCNN_REQUIRE(src_host && dtype_host && ring && marks && totals && state, "journal_append: NULL pointer");
    FRCNN_REQUIRE(((uintptr_t)ring & 7) == 0 && ((uintptr_t)totals & 7) == 0 && ((uintptr_t)marks & 3) == 0 && ((uintptr_t)mark & 3) == 0 &&
                      ((uintptr_t)state & 15) == 0,
                  "journal_append: ring and totals must be 8-byte aligned, marks and mark 4-byte aligned, state 16-byte aligned");
    static const size_t size_of[4] = {4, 8, 4, 8};
    const size_t ring_bytes = (size_t)capacity * (size_t)n_cols * sizeof(double), marks_bytes = (size_t)capacity * sizeof(int32_t);
    const size_t totals_bytes = (size_t)n_cols * sizeof(frcnn_journal_totals);
    JournalArgs a = {};
    for (int c = 0; c <= n_cols; ++c) {                                     // the columns, then the mark word
        const void *src = c < n_cols ? src_host[c] : (const void *)mark;
        size_t b = 4;
        if (c < n_cols) {
            FRCNN_REQUIRE(dtype_host[c] >= 0 && dtype_host[c] <= 3, "journal_append: column %d has the unknown dtype code %d", c, dtype_host[c]);
            b = size_of[dtype_host[c]];
            FRCNN_REQUIRE(src, "journal_append: column %d has a NULL source", c);
            FRCNN_REQUIRE(((uintptr_t)src & (b - 1)) == 0, "journal_append: the source of column %d is not %zu-byte aligned", c, b);
            a.src[c] = src;
            a.dtype[c] = (int8_t)dtype_host[c];
        } else if (!src) {
            break;
        }
        FRCNN_REQUIRE(!tm_overlap(src, b, ring, ring_bytes) && !tm_overlap(src, b, marks, marks_bytes) && !tm_overlap(src, b, totals, totals_bytes) &&
                          !tm_overlap(src, b, state, sizeof(*state)),
                      "journal_append: source %d (%d is the mark word) overlaps ring, marks, totals or state", c, n_cols);
    }
    a.n_cols = n_cols;
    a.capacity = capacity;
    FRCNN_LAUNCH(journal_append_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, a, ring, marks, totals, state, mark);
    FRCNN_CHECK_LAUNCH("journal_append_kernel");
    return FRCNN_OK;
}
