// multi_tensor_dev.h -- what the multi-tensor streaming passes over the optimizer's tensors have in common, once: sgd.hip (the update),
// ema.hip (the weight average and its swap), grad_accum.hip (the accumulation), grad_norm.hip and telemetry.hip (the sums of squares).
// The table layouts and the constants stay in sgd_dev.h / ema_dev.h; the chunk body of the sums of squares stays in sumsq_dev.h.
//
//   host     mt_chunks_of / mt_table_chunks   chunks of a tensor, of a table
//            mt_table                         (table, n_tensors) -> rows and chunk map, const from a const table
//            mt_check_rows                    every row of an op: size in range, no NULL pointer, 4-byte alignment
//            mt_add_span / mt_overlap         nothing that is written may overlap anything else
//   device   mt_chunk                         the workgroup's map entry -> its row, element offset and length; false for a foreign table
//            mt_sweep / mt_chunk_sweep        an index range in sweeps of 4 * SGD_THREADS, every load of a sweep in front of its first store;
//                                             a chunk as 16-byte sweeps over its whole groups of four and dword sweeps over the rest
#pragma once
#include "frcnn_common.h"
#include "sgd_dev.h"
#include <algorithm>
#include <initializer_list>
#include <vector>

constexpr int64_t mt_chunks_of(int64_t numel) { return (numel + SGD_CHUNK - 1) / SGD_CHUNK; }

// The chunks of a table over these tensors; -1 for what the builders refuse: a size outside 0 .. 2^40, more than 2^31 - 1 chunks.
static inline int64_t mt_table_chunks(int n_tensors, const int64_t *numel)
{
    int64_t chunks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 0 || numel[t] > ((int64_t)1 << 40)) return -1;
        chunks += mt_chunks_of(numel[t]);
    }
    return chunks > 0x7fffffff ? -1 : chunks;
}

// Header | Row[n_tensors] | int2 map[n_chunks]: the rows and the chunk map of a table.  From a table that may be written (the builders)
// the pointers are mutable, from a const table (every launch entry point) they are const.
template <class Row, class Map> struct MtTable { Row *rows; Map *map; };
template <class Header, class Row> static inline MtTable<Row, int2> mt_table(void *table, int n_tensors)
{
    char *base = (char *)table;
    return {(Row *)(base + sizeof(Header)), (int2 *)(base + sizeof(Header) + (size_t)n_tensors * sizeof(Row))};
}
template <class Header, class Row> static inline MtTable<const Row, const int2> mt_table(const void *table, int n_tensors)
{
    const MtTable<Row, int2> t = mt_table<Header, Row>(const_cast<void *>(table), n_tensors);
    return {t.rows, t.map};
}

// Every row of `op`: 0 <= numel <= 2^40, and in each of the op's pointer arrays a pointer that is neither NULL nor off a 4-byte boundary.
// All rows are gone through here before a caller's own per-row check (sgd_table_build's group range) sees the first: where one call holds
// several faults, a fault of this list in a later row is reported in front of a group out of range in an earlier one.
static inline int mt_check_rows(const char *op, int n_tensors, const int64_t *numel, std::initializer_list<const void *const *> arrays)
{
    for (int t = 0; t < n_tensors; ++t) {
        FRCNN_REQUIRE(numel[t] >= 0, "%s: tensor %d has a negative size %lld", op, t, (long long)numel[t]);
        FRCNN_REQUIRE(numel[t] <= ((int64_t)1 << 40), "%s: tensor %d is too large (%lld elements)", op, t, (long long)numel[t]);
        bool null = false;
        uintptr_t all = 0;
        for (const void *const *a : arrays) {
            null = null || !a[t];
            all |= (uintptr_t)a[t];
        }
        FRCNN_REQUIRE(!null, "%s: NULL pointer in row %d", op, t);
        FRCNN_REQUIRE((all & 3) == 0, "%s: row %d has a pointer that is not 4-byte aligned", op, t);
    }
    return FRCNN_OK;
}

// The bytes [lo, hi) of one tensor of row `row`; `kind` is the letter the caller's message names it by.
struct Span { uintptr_t lo, hi; int row; char kind; };

static inline void mt_add_span(std::vector<Span> &spans, const void *ptr, int64_t numel, int row, char kind)
{
    const size_t b = (size_t)numel * 4;
    if (b != 0) spans.push_back({(uintptr_t)ptr, (uintptr_t)ptr + b, row, kind});     // an empty tensor overlaps nothing
}

// Nothing that is written may overlap anything else: the written spans pairwise, a read-only span with none of them.  Ranges that only
// touch do not overlap.  Sorts `written`.  what: 0 all disjoint; 1 the written spans a and b overlap (a the lower); 2 the read-only span a
// overlaps a written one.  The written spans are all looked at first, the read-only ones then in their order.
struct MtOverlap { int what; Span a, b; };

static inline MtOverlap mt_overlap(std::vector<Span> &written, const std::vector<Span> &read_only)
{
    std::vector<Span> &w = written;
    std::sort(w.begin(), w.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < w.size(); ++i)
        if (w[i].lo < w[i - 1].hi) return {1, w[i - 1], w[i]};
    for (const Span &r : read_only) {
        auto it = std::upper_bound(w.begin(), w.end(), r.lo, [](uintptr_t v, const Span &s) { return v < s.lo; });
        if ((it != w.end() && it->lo < r.hi) || (it != w.begin() && (it - 1)->hi > r.lo)) return {2, r, r};
    }
    return {0, {}, {}};
}

#ifdef __HIPCC__
// The chunk of this workgroup: its tensor's row, the chunk's first element in the tensor and its 1 .. SGD_CHUNK elements.  false, and *c
// as it was, for a table that is not ours: a tensor number outside 0 .. n_tensors - 1, a negative chunk number, a chunk past the tensor's
// end.  The streaming kernels then touch nothing; the sums of squares start from a zeroed *c (n == 0, NULL pointers: nothing is read).
// Row: SgdRow or EmaRow.
template <class Row> struct MtChunk { Row row; int64_t off; int tensor, n; };

template <class Row>
__device__ __forceinline__ bool mt_chunk(const Row *__restrict__ rows, const int2 *__restrict__ map, int n_tensors, MtChunk<Row> *c)
{
    const int2 e = map[blockIdx.x];
    if ((unsigned)e.x >= (unsigned)n_tensors || e.y < 0) return false;
    const Row r = rows[e.x];
    const int64_t off = (int64_t)e.y * SGD_CHUNK;
    if (off >= r.numel) return false;
    const int64_t left = r.numel - off;
    *c = {r, off, e.x, left < SGD_CHUNK ? (int)left : SGD_CHUNK};
    return true;
}

// The indices lo .. hi - 1 in sweeps of 4 * SGD_THREADS: a thread's four slots of a sweep are SGD_THREADS indices apart.  Slot: the
// caller's registers for one index; load(slot, i) fills them from index i, store(slot, i) computes from them and stores at index i.  The
// four loads are issued before the first store, so four independent accesses per array are in flight per thread.
template <class Slot, class Load, class Store> __device__ __forceinline__ void mt_sweep(int lo, int hi, Load load, Store store)
{
    const int tid = threadIdx.x;
    for (int base = lo; base < hi; base += 4 * SGD_THREADS) {
        Slot r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + k * SGD_THREADS + tid;
            if (i < hi) load(r[k], i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + k * SGD_THREADS + tid;
            if (i < hi) store(r[k], i);
        }
    }
}

// A chunk of n elements.  vec (every pointer of the row is 16-byte aligned; SGD_CHUNK is a multiple of 4, so every chunk of such a row
// starts aligned): load4 / store4 on Slot4 over the n / 4 whole groups of four, indexed in float4, then load1 / store1 on Slot1 over the
// n % 4 elements behind them, indexed in elements.  Otherwise load1 / store1 over all n: the pointers of a row need not share a
// misalignment, so there is no common peel.
template <class Slot4, class Slot1, class Load4, class Store4, class Load1, class Store1>
__device__ __forceinline__ void mt_chunk_sweep(int n, bool vec, Load4 load4, Store4 store4, Load1 load1, Store1 store1)
{
    int done = 0;
    if (vec) {
        mt_sweep<Slot4>(0, n >> 2, load4, store4);
        done = n & ~3;
    }
    mt_sweep<Slot1>(done, n, load1, store1);
}
#endif
