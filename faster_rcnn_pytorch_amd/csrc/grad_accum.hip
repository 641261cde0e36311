// grad_accum.hip -- gradient accumulation over a window of K frames.  The reference takes one optimizer step per frame (train.py:31-37:
// loss.backward(), optimizer.step()) and has no accumulation; the usual recipe sums K backward passes of loss / K into .grad and steps
// once.  Here the sum is ONE multi-tensor launch per group of tensors, and what it does -- write, add, or leave the frame out -- is device
// data (frcnn_grad_accum_state, include/frcnn_hip.h), so a captured graph serves every micro-step of every window.
//
//   p = state->phase, s = frame_skip ? *frame_skip : 0, read once per workgroup:
//                              s == 0                                 s != 0
//   p == 0                     acc = src   (acc is not read)          acc = +0.0f   (neither is read)
//   0 < p < window             acc = __fadd_rn(acc, src)              nothing is read or written
//   p outside 0 .. window-1    nothing is touched                     nothing is touched
//
//   grad_accum_advance_kernel, one thread, the only writer of the state:
//     frames += 1, dropped += (s != 0), live += (s == 0)
//     phase + 1 == window ?  hold = (live == 0), windows += 1, phase = 0, live = 0  :  hold = 1, phase += 1
//
// The sources are autograd's gradient tensors: their addresses exist only inside the capture, where no table can be uploaded.  The
// metadata therefore travels BY VALUE in the kernel arguments, which a graph node stores: GaArgs, GA_ROWS rows of {src, acc, numel, first
// chunk, both-16-byte-aligned bit}, 2.7 KB of the 4 KB argument segment.  One workgroup of SGD_THREADS threads per SGD_CHUNK elements of
// one row; it finds its row by a binary search over the rows' first-chunk numbers -- uniform, so the compiler keeps it in scalar
// registers and reads the argument segment with scalar loads.
//
// Memory: the copy moves 8 B per element, the add 12 B, nothing reused: a streaming kernel.  16-byte accesses when both pointers of a
// row are 16-byte aligned (SGD_CHUNK is a multiple of 4, so every chunk of such a row starts aligned), four independent float4 pairs in
// flight per thread, the source loaded non-temporally (it is read once).  Any other row -- the flat gradient buffers' views start at
// arbitrary element offsets -- takes the dword path for its whole length, four loads in flight per thread.  No atomics, no LDS, no
// workgroup waits on another.  The library is built with -ffp-contract=off; the add is written out (__fadd_rn).
#include "frcnn_common.h"
#include "frcnn_internal.h"
#include "frcnn_layout.h"
#include "sgd_dev.h"
#include "multi_tensor_dev.h"
FRCNN_LAYOUT_STAMP(grad_accum);

#define GA_ROWS FRCNN_GRAD_ACCUM_ROWS
static_assert(GA_ROWS % 32 == 0, "one aligned-bit word per 32 rows");

struct GaArgs {
    const float *src[GA_ROWS];
    float *acc[GA_ROWS];
    int64_t numel[GA_ROWS];
    int32_t first[GA_ROWS];             // the launch-relative number of the row's first chunk; rows in order, empty rows share a number
    uint32_t vec[GA_ROWS / 32];         // bit r: both pointers of row r are 16-byte aligned
    int32_t n_rows, pad;
};
static_assert(sizeof(GaArgs) <= 3072, "GaArgs and the three other arguments must fit well inside the 4 KB kernel-argument segment");

enum { GA_COPY = 0, GA_ZERO = 1, GA_ADD = 2 };

// one index of a sweep (multi_tensor_dev.h): T is sgd_f4 or float.  src and acc are loaded only where the mode reads them.  Zeroed, so that
// no mode reads an undefined register.  In the ISA the zeroing also moves the waits: every slot is written at the head of a sweep, the
// compiler waits there once and issues the sweep's loads back to back; left undefined it puts a wait for the sweep before in front of the
// second and third load.  Both forms were timed once against the parent (profiles/multi_tensor_refactor.json, "ga_regs_zeroed_or_undefined").
template <class T> struct GaRegs { T s = T(0.0f), a = T(0.0f); };

__device__ __forceinline__ float ga_add(float acc, float src) { return __fadd_rn(acc, src); }

__device__ __forceinline__ sgd_f4 ga_add(sgd_f4 acc, sgd_f4 src)
{
    sgd_f4 q;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = __fadd_rn(acc[j], src[j]);
    return q;
}

// the table of the file comment: reads of r only what the mode loaded
template <int MODE, class T> __device__ __forceinline__ T ga_value(const GaRegs<T> &r)
{
    if (MODE == GA_ZERO) return T(0.0f);
    if (MODE == GA_COPY) return r.s;
    return ga_add(r.a, r.s);
}

template <int MODE> __device__ __forceinline__ void ga_chunk(const float *__restrict__ src, float *__restrict__ acc, int n, bool vec)
{
    sgd_f4 *a4 = (sgd_f4 *)acc;
    const sgd_f4 *s4 = (const sgd_f4 *)src;
    mt_chunk_sweep<GaRegs<sgd_f4>, GaRegs<float>>(
        n, vec,
        [&](GaRegs<sgd_f4> &r, int i) {
            if (MODE != GA_ZERO) r.s = __builtin_nontemporal_load(&s4[i]);
            if (MODE == GA_ADD) r.a = a4[i];
        },
        [&](GaRegs<sgd_f4> &r, int i) { a4[i] = ga_value<MODE>(r); },
        [&](GaRegs<float> &r, int i) {                                      // the tail of an aligned row; all of a misaligned one
            if (MODE != GA_ZERO) r.s = __builtin_nontemporal_load(&src[i]);
            if (MODE == GA_ADD) r.a = acc[i];
        },
        [&](GaRegs<float> &r, int i) { acc[i] = ga_value<MODE>(r); });
}

__global__ __launch_bounds__(SGD_THREADS) void grad_accum_kernel(const GaArgs a, const frcnn_grad_accum_state *__restrict__ st,
                                                                const int32_t *__restrict__ frame_skip)
{
    const int p = st->phase, w = st->window;
    const int s = frame_skip ? *frame_skip : 0;
    if (p < 0 || p >= w) return;                                            // a state that is not ours: touch nothing
    if (p > 0 && s != 0) return;                                            // a later frame that is left out: before any load of src or acc
    const int c = (int)blockIdx.x;
    int lo = 0, hi = a.n_rows;                                              // the last row whose first chunk is <= c (an empty row never is)
    if (hi < 1 || hi > GA_ROWS) return;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first[mid] <= c) lo = mid;
        else hi = mid;
    }
    const int64_t off = (int64_t)(c - a.first[lo]) * SGD_CHUNK;
    const int64_t numel = a.numel[lo];
    if (off < 0 || off >= numel) return;
    const int64_t left = numel - off;
    const int n = left < SGD_CHUNK ? (int)left : SGD_CHUNK;
    const float *src = a.src[lo] + off;
    float *acc = a.acc[lo] + off;
    const bool vec = (a.vec[lo >> 5] >> (lo & 31)) & 1u;
    if (p > 0) ga_chunk<GA_ADD>(src, acc, n, vec);
    else if (s != 0) ga_chunk<GA_ZERO>(src, acc, n, vec);
    else ga_chunk<GA_COPY>(src, acc, n, vec);
}

__global__ __launch_bounds__(WAVE) void grad_accum_advance_kernel(frcnn_grad_accum_state *__restrict__ st, const int32_t *__restrict__ frame_skip)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int p = st->phase, w = st->window;
    if (p < 0 || p >= w) return;                                            // a state that is not ours: touch nothing
    const int s = frame_skip ? *frame_skip : 0;
    const int live = st->live + (s == 0);
    st->frames = st->frames + 1;
    st->dropped = st->dropped + (s != 0);
    if (p + 1 == w) {
        st->hold = live == 0;
        st->windows = st->windows + 1;
        st->phase = 0;
        st->live = 0;
    } else {
        st->hold = 1;
        st->phase = p + 1;
        st->live = live;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
FRCNN_EXPORT int frcnn_grad_accum_rows_per_launch(void) { return GA_ROWS; }

// train.py:31-37 (what K backward passes leave in .grad in front of ONE optimizer.step()).  ceil(n_tensors / GA_ROWS) launches at most,
// fixed by the tensor list; no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_grad_accumulate(int n_tensors, const void *const *src_host, void *const *acc_host, const int64_t *numel_host,
                                       const frcnn_grad_accum_state *state, const int32_t *frame_skip, void *stream)
{
    FRCNN_REQUIRE(src_host && acc_host && numel_host && state, "grad_accumulate: NULL argument");
    FRCNN_REQUIRE(n_tensors >= 1 && n_tensors <= SGD_MAX_TENSORS, "grad_accumulate: n_tensors %d outside 1 .. %d", n_tensors, SGD_MAX_TENSORS);
    FRCNN_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)frame_skip & 3) == 0,
                  "grad_accumulate: state must be 16-byte aligned, frame_skip 4-byte aligned");
    const int rc = mt_check_rows("grad_accumulate", n_tensors, numel_host, {src_host, (const void *const *)acc_host});
    if (rc != FRCNN_OK) return rc;
    // written: the acc ranges; read only: the src ranges
    std::vector<Span> w, ro;
    for (int t = 0; t < n_tensors; ++t) {
        mt_add_span(w, acc_host[t], numel_host[t], t, 'a');
        mt_add_span(ro, src_host[t], numel_host[t], t, 's');
    }
    const MtOverlap o = mt_overlap(w, ro);
    FRCNN_REQUIRE(o.what != 1, "grad_accumulate: overlapping acc ranges (rows %d and %d)", o.a.row, o.b.row);
    FRCNN_REQUIRE(o.what != 2, "grad_accumulate: the src of row %d overlaps an acc range", o.a.row);
    for (int t0 = 0; t0 < n_tensors; t0 += GA_ROWS) {                       // every launch's chunk count, before the first launch
        int64_t chunks = 0;
        for (int t = t0; t < n_tensors && t < t0 + GA_ROWS; ++t) chunks += mt_chunks_of(numel_host[t]);
        FRCNN_REQUIRE(chunks <= 0x7fffffff, "grad_accumulate: rows %d .. hold more than 2^31 - 1 chunks", t0);
    }
    hipStream_t s = (hipStream_t)stream;
    bool launched = false;
    for (int t0 = 0; t0 < n_tensors; t0 += GA_ROWS) {
        GaArgs a = {};
        const int rows = std::min(GA_ROWS, n_tensors - t0);
        int64_t chunks = 0;
        for (int r = 0; r < rows; ++r) {
            const int t = t0 + r;
            a.src[r] = (const float *)src_host[t];
            a.acc[r] = (float *)acc_host[t];
            a.numel[r] = numel_host[t];
            a.first[r] = (int32_t)chunks;
            if ((((uintptr_t)src_host[t] | (uintptr_t)acc_host[t]) & 15) == 0) a.vec[r >> 5] |= 1u << (r & 31);
            chunks += mt_chunks_of(numel_host[t]);
        }
        a.n_rows = rows;
        if (chunks == 0) continue;                                          // every tensor of this launch is empty
        FRCNN_LAUNCH(grad_accum_kernel, dim3((unsigned)chunks), dim3(SGD_THREADS), 0, s, a, state, frame_skip);
        launched = true;
    }
    if (!launched) return FRCNN_OK;                                         // every tensor is empty: the runtime is not touched
    FRCNN_CHECK_LAUNCH("grad_accum_kernel");
    return FRCNN_OK;
}

// The bookkeeping of train.py:31-37 run K times per optimizer.step(): one launch of one thread, no host synchronisation, capturable.
FRCNN_EXPORT int frcnn_grad_accum_advance(frcnn_grad_accum_state *state, const int32_t *frame_skip, void *stream)
{
    FRCNN_REQUIRE(state, "grad_accum_advance: NULL state");
    FRCNN_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)frame_skip & 3) == 0,
                  "grad_accum_advance: state must be 16-byte aligned, frame_skip 4-byte aligned");
    FRCNN_LAUNCH(grad_accum_advance_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, state, frame_skip);
    FRCNN_CHECK_LAUNCH("grad_accum_advance_kernel");
    return FRCNN_OK;
}
