// eval_merge.hip -- the image ledger of the device evaluators and the merge of their shards across ranks: what the reference's
// distributed test loop does on the host (test.py:60-128; evaluation/coco_eval.py:46-49 synchronize_between_processes, :161-190 merge:
// all_gather, then np.unique(img_ids, return_index=True) keeps the FIRST occurrence of every image id), on the device and with no host sync.
//
//  eval_ledger_append_kernel : one workgroup after an update kernel on the same stream.  One ledger row per frame: image_id (frame[2]),
//      the record slots [cursor snapshot, cursor) the frame took, and delta = counter - counter snapshot as int32; then the snapshots are
//      replaced.  The kernel knows nothing of either protocol's counting rule.  A full ledger keeps counting and sets EVAL_ERR_LEDGER_OVERFLOW.
//
//  frcnn_eval_merge : W shards, one padded buffer per column [W, shard capacity, ...], live counts in device memory.  An occurrence is
//      (shard, ledger row), ordered by g = shard * shard_image_capacity + row; it is KEPT iff no earlier occurrence has its image_id.  Eight
//      launches whatever the data, none of which waits for another workgroup:
//        1 merge_init_kernel     the table of the dedupe to EMPTY, the destination counter to zero
//        2 merge_insert_kernel   open addressing, slot = id mod table size, linear probing: a slot is claimed with one compare-and-swap of
//                                (id << 32 | g) and lowered with a 64-bit atomic min, so after the launch it holds the id's FIRST g -- a
//                                minimum, hence deterministic whatever the order of arrival.  Every int32 is a legal id: EMPTY is all ones,
//                                which is no key because g < 2^31.  The table has at least twice as many slots as occurrences.
//        3 merge_keep_kernel     keep flag of every occurrence; per workgroup of MERGE_ROW_BLOCK rows the kept rows and their records
//        4 merge_flag_kernel     every record finds its occurrence by bisection over its shard's row ranges and takes that row's flag;
//                                per workgroup of MERGE_SCAN_BLOCK records the number kept
//        5 merge_scan_kernel     ONE workgroup: exclusive scans of the three arrays of block counts; cursor, ledger count, error word
//        6 merge_scatter_kernel  the hot loop, 32 B (COCO: 44 B) per kept record: 16-byte loads of four consecutive records per lane and
//                                column, order-preserving compaction in LDS, 16-byte stores of the workgroup's contiguous run; a COCO
//                                record's four flag words travel as one 16-byte access, consecutive lanes on consecutive records
//        7 merge_ledger_kernel   kept rows with rebased ranges, their delta rows, and the counter: one int64 atomic add per (workgroup,
//                                counter word) -- integer sums, the same in any order
//        8 merge_finish_kernel   the snapshots of the destination follow its counter and cursor, so that update() may go on after a merge
//      Records of kept occurrences land in (shard, slot) order, all five columns bit for bit.  Row ranges are read from device memory and
//      clipped to the shard's live records before they index anything.
#include "frcnn_common.h"
#include "frcnn_dev.h"
#include "frcnn_layout.h"
#include "eval_dev.h"
FRCNN_LAYOUT_STAMP(eval_merge);

#define MERGE_THREADS 256
#define MERGE_SCAN_BLOCK 1024          // records per workgroup of the compaction: MERGE_THREADS lanes x 4 records
#define MERGE_ROW_BLOCK 256            // ledger rows per workgroup: one per lane
#define MERGE_MAX_W 64
#define MERGE_MAX_WORDS (4 * (EVAL_MAX_C - 1))
#define MERGE_EMPTY 0xFFFFFFFFFFFFFFFFull

struct MergeSrc {
    const int32_t *score, *label, *image, *order;              // [W, SR]; the score travels as its bit pattern
    const uint32_t *flags;                                      // [W, SR, FW]
    const int32_t *led_image;                                   // [W, SI]
    const long long *led_range;                                 // [W, SI, 2]
    const int32_t *led_delta;                                   // [W, SI, CW]
    const long long *n_rec, *n_img;                             // [W] on the device
    const int32_t *err;                                         // [W]
    int W, SR, SI, CW;
};

struct MergeDst {
    int32_t *score, *label, *image, *order;
    uint32_t *flags;
    int32_t *led_image;
    long long *led_range;
    int32_t *led_delta;
    long long RC, IC;
    u64 *counter;
    long long *cursor, *led_count;
    int32_t *err;
    long long *snap_cursor, *snap_counter;
};

struct MergeWs { u64 *table; long long TS; uint8_t *keep_row, *keep_rec; u64 *rb, *lb_cnt, *lb_len; long long NB1, NB2; };

static long long merge_table_slots(int64_t n2)
{
    long long ts = 64;
    while (ts < 2 * (long long)n2) ts <<= 1;
    return ts;
}

// n1 = W * SR, n2 = W * SI.  The block-count arrays are sized for the most workgroups W <= 64 shards can need: n / block + 64.
// Returns the bytes; MergeWs itself is a kernel argument and holds no host-side total.
static size_t merge_ws_layout(int64_t n1, int64_t n2, void *workspace, MergeWs *w)
{
    const long long nb1 = n1 / MERGE_SCAN_BLOCK + MERGE_MAX_W, nb2 = n2 / MERGE_ROW_BLOCK + MERGE_MAX_W;
    WsCarver c = WsCarver::any_base(workspace);
    w->TS = merge_table_slots(n2);
    w->table = c.get<u64>((size_t)w->TS);
    w->keep_row = c.get<uint8_t>((size_t)n2 + 1);
    w->keep_rec = c.get<uint8_t>((size_t)n1 + 4);
    w->rb = c.get<u64>((size_t)nb1);
    w->lb_cnt = c.get<u64>((size_t)nb2);
    w->lb_len = c.get<u64>((size_t)nb2);
    return c.bytes();
}

static bool merge_supported(int64_t n1, int64_t n2) { return n1 >= 0 && n2 >= 0 && n1 < ((int64_t)1 << 31) - 4096 && n2 < ((int64_t)1 << 30); }

size_t frcnn_ws_eval_merge(int64_t n1, int64_t n2)
{
    MergeWs w;
    return merge_supported(n1, n2) ? merge_ws_layout(n1, n2, nullptr, &w) : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the ledger
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MERGE_THREADS) void eval_ledger_append_kernel(
    const int32_t *__restrict__ frame, const long long *__restrict__ cursor, const long long *__restrict__ counter, int CW,
    long long *__restrict__ snap_cursor, long long *__restrict__ snap_counter, int32_t *__restrict__ led_image, long long *__restrict__ led_range,
    int32_t *__restrict__ led_delta, long long IC, long long *__restrict__ led_count, int32_t *__restrict__ err)
{
    const int tid = threadIdx.x;
    const long long row = *led_count;                           // one workgroup, stream-ordered: no other writer
    const bool room = row >= 0 && row < IC;
    for (int w = tid; w < CW; w += MERGE_THREADS) {
        const long long c = counter[w];
        const long long d = c - snap_counter[w];
        snap_counter[w] = c;
        if (room) led_delta[(size_t)row * CW + w] = (int32_t)d;
    }
    __syncthreads();                                            // every lane has read *led_count
    if (tid == 0) {
        const long long now = *cursor;
        if (room) {
            led_image[row] = frame[2];
            led_range[2 * row] = *snap_cursor;
            led_range[2 * row + 1] = now;
        } else {
            atomicOr(err, EVAL_ERR_LEDGER_OVERFLOW);
        }
        *snap_cursor = now;
        *led_count = row + 1;                                   // a full ledger keeps counting: summarize() reports the loss
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the merge
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int merge_live(const long long *__restrict__ n, int w, int cap)
{
    const long long v = n[w];
    return v < 0 ? 0 : (v > cap ? cap : (int)v);
}

// the row's record range clipped to the shard's live records: 0 <= b <= e <= nrec
__device__ __forceinline__ void merge_range(const long long *__restrict__ rng, long long g, int nrec, int &b, int &e)
{
    long long lb = rng[2 * g], le = rng[2 * g + 1];
    lb = lb < 0 ? 0 : (lb > nrec ? nrec : lb);
    le = le < lb ? lb : (le > nrec ? nrec : le);
    b = (int)lb;
    e = (int)le;
}

// block-wide inclusive scan of one u64 per lane; s_wave holds MERGE_THREADS / 64 words (the next scan's first barrier guards their reuse);
// *total = the block's sum.
__device__ __forceinline__ u64 merge_block_scan(u64 v, u64 *s_wave, u64 *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    v = wave_incl_scan(v);
    __syncthreads();                                            // s_wave of an earlier scan has been read
    if (lane == 63) s_wave[wv] = v;
    __syncthreads();
    u64 pre = 0, tot = 0;
    for (int w = 0; w < MERGE_THREADS / 64; ++w) {
        if (w < wv) pre += s_wave[w];
        tot += s_wave[w];
    }
    *total = tot;
    return v + pre;
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_init_kernel(u64 *__restrict__ table, long long TS, u64 *__restrict__ counter, int CW)
{
    const long long i0 = (long long)blockIdx.x * MERGE_THREADS + threadIdx.x, step = (long long)gridDim.x * MERGE_THREADS;
    for (long long i = i0; i < TS; i += step) table[i] = MERGE_EMPTY;
    for (long long i = i0; i < CW; i += step) counter[i] = 0ull;
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_insert_kernel(MergeSrc s, u64 *__restrict__ table, long long TS)
{
    const long long g = (long long)blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (g >= (long long)s.W * s.SI) return;
    const int w = (int)(g / s.SI), r = (int)(g % s.SI);
    if (r >= merge_live(s.n_img, w, s.SI)) return;
    const uint32_t id = (uint32_t)s.led_image[g];
    const u64 key = ((u64)id << 32) | (u64)(uint32_t)g;
    const u64 mask = (u64)TS - 1;
    u64 h = (u64)id & mask;
    for (long long probe = 0; probe < TS; ++probe) {            // the table is at most half full: an empty or the id's own slot is met
        u64 cur = agent_ld(&table[h]);
        if (cur == MERGE_EMPTY) {
            cur = atomicCAS(&table[h], MERGE_EMPTY, key);
            if (cur == MERGE_EMPTY) return;                     // claimed
        }
        if ((uint32_t)(cur >> 32) == id) {                      // a slot never changes its id: lower it to the first occurrence
            atomicMin(&table[h], key);
            return;
        }
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_keep_kernel(MergeSrc s, const u64 *__restrict__ table, long long TS,
                                                                    uint8_t *__restrict__ keep_row, u64 *__restrict__ lb_cnt, u64 *__restrict__ lb_len)
{
    __shared__ u64 s_wave[MERGE_THREADS / 64];
    const int tps = (s.SI + MERGE_ROW_BLOCK - 1) / MERGE_ROW_BLOCK;
    const int w = blockIdx.x / tps, r = (blockIdx.x % tps) * MERGE_ROW_BLOCK + threadIdx.x;
    u64 v = 0;
    if (r < s.SI) {
        const long long g = (long long)w * s.SI + r;
        uint32_t keep = 0;
        if (r < merge_live(s.n_img, w, s.SI)) {
            const uint32_t id = (uint32_t)s.led_image[g];
            const u64 mask = (u64)TS - 1;
            u64 h = (u64)id & mask;
            for (long long probe = 0; probe < TS; ++probe) {
                const u64 cur = table[h];
                if (cur == MERGE_EMPTY) break;                  // not met: every live occurrence was inserted by the launch before
                if ((uint32_t)(cur >> 32) == id) { keep = (uint32_t)cur == (uint32_t)g; break; }
                h = (h + 1) & mask;
            }
            if (keep) {
                int b, e;
                merge_range(s.led_range, g, merge_live(s.n_rec, w, s.SR), b, e);
                v = ((u64)(uint32_t)(e - b) << 32) | 1ull;      // records in the high half, rows in the low half
            }
        }
        keep_row[g] = (uint8_t)keep;
    }
    u64 tot;
    merge_block_scan(v, s_wave, &tot);
    if (threadIdx.x == 0) {
        lb_cnt[blockIdx.x] = tot & 0xffffffffull;
        lb_len[blockIdx.x] = tot >> 32;
    }
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_flag_kernel(MergeSrc s, const uint8_t *__restrict__ keep_row, uint8_t *__restrict__ keep_rec,
                                                                    u64 *__restrict__ rb)
{
    __shared__ u64 s_wave[MERGE_THREADS / 64];
    const int tps = (s.SR + MERGE_SCAN_BLOCK - 1) / MERGE_SCAN_BLOCK;
    const int w = blockIdx.x / tps, i0 = (blockIdx.x % tps) * MERGE_SCAN_BLOCK + 4 * threadIdx.x;
    u64 c = 0;
    if (i0 < s.SR) {                                            // SR is a multiple of 4: the four records are inside the shard's buffer
        const int nrec = merge_live(s.n_rec, w, s.SR), nimg = merge_live(s.n_img, w, s.SI);
        const long long g0 = (long long)w * s.SI;
        int b = 0, e = 0;                                       // the range found last and its flag
        uint32_t f = 0, word = 0;
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k;
            uint32_t fk = 0;
            if (i < nrec) {
                if (i < b || i >= e) {                          // the last row whose range begins at or before i
                    int lo = 0, hi = nimg;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        int mb, me;
                        merge_range(s.led_range, g0 + mid, nrec, mb, me);
                        if (mb <= i) lo = mid + 1; else hi = mid;
                    }
                    b = e = 0;
                    f = 0;
                    if (lo > 0) {
                        merge_range(s.led_range, g0 + lo - 1, nrec, b, e);
                        f = keep_row[g0 + lo - 1];
                    }
                }
                if (i >= b && i < e) fk = f;
            }
            word |= fk << (8 * k);
            c += fk;
        }
        *(uint32_t *)(keep_rec + (size_t)w * s.SR + i0) = word;
    }
    u64 tot;
    merge_block_scan(c, s_wave, &tot);
    if (threadIdx.x == 0) rb[blockIdx.x] = tot;
}

// exclusive scan of a[0 .. n) in place by ONE workgroup; returns the total
__device__ __forceinline__ u64 merge_scan_array(u64 *__restrict__ a, long long n, u64 *s_wave)
{
    u64 carry = 0;
    for (long long c0 = 0; c0 < n; c0 += MERGE_THREADS) {
        const long long i = c0 + threadIdx.x;
        const u64 v = i < n ? a[i] : 0ull;
        u64 tot;
        const u64 inc = merge_block_scan(v, s_wave, &tot);
        if (i < n) a[i] = carry + inc - v;
        carry += tot;
    }
    return carry;
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_scan_kernel(MergeSrc s, MergeDst d, u64 *__restrict__ rb, long long NB1, u64 *__restrict__ lb_cnt,
                                                                    u64 *__restrict__ lb_len, long long NB2)
{
    __shared__ u64 s_wave[MERGE_THREADS / 64];
    const u64 n_rec = merge_scan_array(rb, NB1, s_wave);
    const u64 n_img = merge_scan_array(lb_cnt, NB2, s_wave);
    merge_scan_array(lb_len, NB2, s_wave);
    u64 e = 0;
    if (threadIdx.x < s.W) {
        e = (u64)(uint32_t)s.err[threadIdx.x];
        if (s.n_rec[threadIdx.x] > s.SR || s.n_img[threadIdx.x] > s.SI) e |= EVAL_ERR_SHARD_TRUNCATED;     // the shard had lost some already
    }
    for (int o = 1; o < 64; o <<= 1) e |= __shfl_xor(e, o);     // W <= 64: the first wave holds every shard's word
    if (threadIdx.x == 0) {
        *d.cursor = (long long)n_rec;                           // beyond RC too: summarize() reports the loss
        *d.led_count = (long long)n_img;
        *d.err = (int32_t)(uint32_t)e | ((long long)n_img > d.IC ? EVAL_ERR_LEDGER_OVERFLOW : 0);
        *d.snap_cursor = (long long)n_rec;
    }
}

// One dword column of the workgroup's run: n values in LDS go to dst[o .. o + n), cut at RC.  Lane j owns the 16-byte aligned quad
// (o / 4 + j) of the destination: one 16-byte store where the quad lies inside the run, dword stores at the run's two ends.
__device__ __forceinline__ void merge_store_run(int32_t *__restrict__ dst, const int32_t *s_v, long long o, int n, long long RC)
{
    long long end = o + n;
    if (end > RC) end = RC;
    const long long q0 = o >> 2, q1 = (end + 3) >> 2;
    for (long long q = q0 + threadIdx.x; q < q1; q += MERGE_THREADS) {
        const long long p = q << 2;
        if (p >= o && p + 4 <= end) {
            const int j = (int)(p - o);
            *(int4 *)(dst + p) = make_int4(s_v[j], s_v[j + 1], s_v[j + 2], s_v[j + 3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (p + k >= o && p + k < end) dst[p + k] = s_v[(int)(p + k - o)];
        }
    }
}

template <int FW>
__global__ __launch_bounds__(MERGE_THREADS) void merge_scatter_kernel(MergeSrc s, MergeDst d, const uint8_t *__restrict__ keep_rec,
                                                                       const u64 *__restrict__ rb)
{
    __shared__ int32_t s_col[4][MERGE_SCAN_BLOCK];
    __shared__ int4 s_f4[FW == 4 ? MERGE_SCAN_BLOCK : 1];
    __shared__ int32_t s_f1[FW == 1 ? MERGE_SCAN_BLOCK : 1];
    __shared__ int32_t s_loff[FW == 4 ? MERGE_SCAN_BLOCK : 4];
    __shared__ u64 s_wave[MERGE_THREADS / 64];
    const int tid = threadIdx.x;
    const int tps = (s.SR + MERGE_SCAN_BLOCK - 1) / MERGE_SCAN_BLOCK;
    const int w = blockIdx.x / tps, t0 = (blockIdx.x % tps) * MERGE_SCAN_BLOCK, i0 = t0 + 4 * tid;
    const size_t base = (size_t)w * s.SR;
    const bool in = i0 < s.SR;
    const uint32_t word = in ? *(const uint32_t *)(keep_rec + base + i0) : 0u;
    const u64 c = (word & 1u) + ((word >> 8) & 1u) + ((word >> 16) & 1u) + ((word >> 24) & 1u);
    u64 tot;
    int off = (int)(merge_block_scan(c, s_wave, &tot) - c);
    const int n = (int)tot;
    if (n == 0) return;                                         // uniform: the whole workgroup leaves
    int4 lo4 = make_int4(-1, -1, -1, -1);
    if (c) {
        const int4 a = *(const int4 *)(s.score + base + i0), b = *(const int4 *)(s.label + base + i0);
        const int4 e = *(const int4 *)(s.image + base + i0), f = *(const int4 *)(s.order + base + i0);
        int4 g = make_int4(0, 0, 0, 0);
        if (FW == 1) g = *(const int4 *)(s.flags + base + i0);
        const int av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w}, ev[4] = {e.x, e.y, e.z, e.w}, fv[4] = {f.x, f.y, f.z, f.w};
        const int gv[4] = {g.x, g.y, g.z, g.w};
        int lv[4] = {-1, -1, -1, -1};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((word >> (8 * k)) & 1u) {
                s_col[0][off] = av[k]; s_col[1][off] = bv[k]; s_col[2][off] = ev[k]; s_col[3][off] = fv[k];
                if (FW == 1) s_f1[off] = gv[k];
                lv[k] = off++;
            }
        lo4 = make_int4(lv[0], lv[1], lv[2], lv[3]);
    }
    if (FW == 4) {
        *(int4 *)&s_loff[4 * tid] = lo4;
        __syncthreads();
        const int4 *src = (const int4 *)s.flags + base + t0;    // consecutive lanes on consecutive records: one 16-byte load each
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = k * MERGE_THREADS + tid;
            const int l = s_loff[j];
            if (l >= 0) s_f4[l] = src[j];
        }
    }
    __syncthreads();
    const long long o = (long long)rb[blockIdx.x];
    merge_store_run(d.score, s_col[0], o, n, d.RC);
    merge_store_run(d.label, s_col[1], o, n, d.RC);
    merge_store_run(d.image, s_col[2], o, n, d.RC);
    merge_store_run(d.order, s_col[3], o, n, d.RC);
    if (FW == 1) {
        merge_store_run((int32_t *)d.flags, s_f1, o, n, d.RC);
    } else {
        int4 *dst = (int4 *)d.flags;
        for (int j = tid; j < n; j += MERGE_THREADS)
            if (o + j < d.RC) dst[o + j] = s_f4[j];
    }
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_ledger_kernel(MergeSrc s, MergeDst d, const uint8_t *__restrict__ keep_row,
                                                                      const u64 *__restrict__ lb_cnt, const u64 *__restrict__ lb_len)
{
    __shared__ u64 s_wave[MERGE_THREADS / 64];
    __shared__ int32_t s_row[MERGE_ROW_BLOCK];                  // the kept rows of the tile, in order: their index in the shard
    const int tid = threadIdx.x;
    const int tps = (s.SI + MERGE_ROW_BLOCK - 1) / MERGE_ROW_BLOCK;
    const int w = blockIdx.x / tps, r = (blockIdx.x % tps) * MERGE_ROW_BLOCK + tid;
    const long long g0 = (long long)w * s.SI;
    u64 v = 0;
    int b = 0, e = 0;
    if (r < s.SI && keep_row[g0 + r]) {
        merge_range(s.led_range, g0 + r, merge_live(s.n_rec, w, s.SR), b, e);
        v = ((u64)(uint32_t)(e - b) << 32) | 1ull;
    }
    u64 tot;
    const u64 ex = merge_block_scan(v, s_wave, &tot) - v;
    const int n = (int)(tot & 0xffffffffull);
    if (n == 0) return;                                         // uniform
    const long long row0 = (long long)lb_cnt[blockIdx.x];
    if (v) {
        const int l = (int)(ex & 0xffffffffull);
        s_row[l] = r;
        const long long dr = row0 + l;
        if (dr < d.IC) {
            const long long nb = (long long)lb_len[blockIdx.x] + (long long)(ex >> 32);
            d.led_image[dr] = s.led_image[g0 + r];
            d.led_range[2 * dr] = nb;
            d.led_range[2 * dr + 1] = nb + (e - b);
        }
    }
    __syncthreads();
    for (int wd = tid; wd < s.CW; wd += MERGE_THREADS) {        // consecutive lanes on consecutive words of a row
        long long sum = 0;
        for (int j = 0; j < n; ++j) {
            const int32_t dv = s.led_delta[(size_t)(g0 + s_row[j]) * s.CW + wd];
            sum += dv;
            if (row0 + j < d.IC) d.led_delta[(size_t)(row0 + j) * s.CW + wd] = dv;
        }
        if (sum) atomicAdd(&d.counter[wd], (u64)sum);           // two's complement: a negative delta subtracts
    }
}

__global__ __launch_bounds__(MERGE_THREADS) void merge_finish_kernel(const u64 *__restrict__ counter, long long *__restrict__ snap_counter, int CW)
{
    const int i = blockIdx.x * MERGE_THREADS + threadIdx.x;
    if (i < CW) snap_counter[i] = (long long)counter[i];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------------------------------------------
FRCNN_EXPORT int frcnn_eval_ledger_append(const int32_t *frame_dev, const int64_t *cursor, const int64_t *counter, int64_t counter_words,
                                          int64_t *snap_cursor, int64_t *snap_counter, int32_t *led_image, int64_t *led_range, int32_t *led_delta,
                                          int64_t image_capacity, int64_t *led_count, int32_t *error_word, void *stream)
{
    FRCNN_REQUIRE(frame_dev && cursor && counter && snap_cursor && snap_counter && led_image && led_range && led_delta && led_count && error_word,
                  "eval_ledger_append: NULL pointer");
    FRCNN_REQUIRE(image_capacity >= 1, "eval_ledger_append: image_capacity must be >= 1");
    if (counter_words < 1 || counter_words > MERGE_MAX_WORDS)
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "eval_ledger_append: %lld counter words outside 1 .. %d", (long long)counter_words, MERGE_MAX_WORDS);
    hipStream_t s = (hipStream_t)stream;
    FRCNN_LAUNCH(eval_ledger_append_kernel, dim3(1), dim3(MERGE_THREADS), 0, s, frame_dev, (const long long *)cursor, (const long long *)counter,
                 (int)counter_words, (long long *)snap_cursor, (long long *)snap_counter, led_image, (long long *)led_range, led_delta,
                 (long long)image_capacity, (long long *)led_count, error_word);
    FRCNN_CHECK_LAUNCH("eval_ledger_append_kernel");
    return FRCNN_OK;
}

struct MergeSpan { const void *p; size_t bytes; };
static bool merge_overlap(const MergeSpan &a, const MergeSpan &b)
{
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.bytes && b.bytes && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

FRCNN_EXPORT int frcnn_eval_merge(int W, int64_t shard_record_capacity, int64_t shard_image_capacity, int flags_width, int64_t counter_words,
                                  const float *sh_score, const int32_t *sh_label, const int32_t *sh_image, const int32_t *sh_order,
                                  const uint32_t *sh_flags, const int32_t *sh_led_image, const int64_t *sh_led_range, const int32_t *sh_led_delta,
                                  const int64_t *sh_n_records, const int64_t *sh_n_images, const int32_t *sh_error, float *rec_score,
                                  int32_t *rec_label, int32_t *rec_image, int32_t *rec_order, uint32_t *rec_flags, int64_t record_capacity,
                                  int32_t *led_image, int64_t *led_range, int32_t *led_delta, int64_t image_capacity, int64_t *counter,
                                  int64_t *cursor, int64_t *led_count, int32_t *error_word, int64_t *snap_cursor, int64_t *snap_counter,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    FRCNN_REQUIRE(sh_score && sh_label && sh_image && sh_order && sh_flags && sh_led_image && sh_led_range && sh_led_delta && sh_n_records &&
                  sh_n_images && sh_error && rec_score && rec_label && rec_image && rec_order && rec_flags && led_image && led_range && led_delta &&
                  counter && cursor && led_count && error_word && snap_cursor && snap_counter && workspace, "eval_merge: NULL pointer");
    if (W < 1 || W > MERGE_MAX_W) return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "eval_merge: %d shards outside 1 .. %d", W, MERGE_MAX_W);
    FRCNN_REQUIRE(shard_record_capacity >= 0 && shard_image_capacity >= 0 && record_capacity >= 0 && image_capacity >= 0,
                  "eval_merge: negative capacity");
    FRCNN_REQUIRE(flags_width == 1 || flags_width == 4, "eval_merge: flags_width %d, 1 (VOC) or 4 (COCO) supported", flags_width);
    FRCNN_REQUIRE(shard_record_capacity % 4 == 0, "eval_merge: shard_record_capacity %lld must be a multiple of 4 (16-byte accesses)",
                  (long long)shard_record_capacity);
    const int64_t SR = shard_record_capacity, SI = shard_image_capacity, n1 = (int64_t)W * SR, n2 = (int64_t)W * SI;
    if (counter_words < 1 || counter_words > MERGE_MAX_WORDS || !merge_supported(n1, n2))
        return frcnn_set_error(FRCNN_ERR_UNSUPPORTED, "eval_merge: %lld counter words, %lld shard records, %lld shard images outside 1 .. %d, "
                               "W * records < 2^31 - 4096, W * images < 2^30", (long long)counter_words, (long long)n1, (long long)n2, MERGE_MAX_WORDS);
    const size_t FW = (size_t)flags_width, CW = (size_t)counter_words;
    const MergeSpan src[] = {{sh_score, 4 * (size_t)n1}, {sh_label, 4 * (size_t)n1}, {sh_image, 4 * (size_t)n1}, {sh_order, 4 * (size_t)n1},
                             {sh_flags, 4 * FW * (size_t)n1}, {sh_led_image, 4 * (size_t)n2}, {sh_led_range, 16 * (size_t)n2},
                             {sh_led_delta, 4 * CW * (size_t)n2}, {sh_n_records, 8 * (size_t)W}, {sh_n_images, 8 * (size_t)W}, {sh_error, 4 * (size_t)W}};
    const MergeSpan dst[] = {{rec_score, 4 * (size_t)record_capacity}, {rec_label, 4 * (size_t)record_capacity}, {rec_image, 4 * (size_t)record_capacity},
                             {rec_order, 4 * (size_t)record_capacity}, {rec_flags, 4 * FW * (size_t)record_capacity}, {led_image, 4 * (size_t)image_capacity},
                             {led_range, 16 * (size_t)image_capacity}, {led_delta, 4 * CW * (size_t)image_capacity}, {counter, 8 * CW}, {cursor, 8},
                             {led_count, 8}, {error_word, 4}, {snap_cursor, 8}, {snap_counter, 8 * CW}};
    for (int i = 0; i < 5; ++i)
        FRCNN_REQUIRE(((uintptr_t)src[i].p & 15) == 0 && ((uintptr_t)dst[i].p & 15) == 0, "eval_merge: the record columns must be 16-byte aligned");
    FRCNN_REQUIRE(((uintptr_t)sh_led_range & 7) == 0 && ((uintptr_t)led_range & 7) == 0 && ((uintptr_t)sh_n_records & 7) == 0 &&
                  ((uintptr_t)sh_n_images & 7) == 0 && ((uintptr_t)counter & 7) == 0 && ((uintptr_t)cursor & 7) == 0 && ((uintptr_t)led_count & 7) == 0 &&
                  ((uintptr_t)snap_cursor & 7) == 0 && ((uintptr_t)snap_counter & 7) == 0, "eval_merge: the 64-bit buffers must be 8-byte aligned");
    MergeWs ws;
    FRCNN_REQUIRE_WS("eval_merge", workspace_bytes, merge_ws_layout(n1, n2, workspace, &ws));
    const MergeSpan wsp = {workspace, workspace_bytes};
    const int ns = (int)(sizeof(src) / sizeof(src[0])), nd = (int)(sizeof(dst) / sizeof(dst[0]));
    for (int i = 0; i < nd; ++i) {
        FRCNN_REQUIRE(!merge_overlap(dst[i], wsp), "eval_merge: a destination buffer overlaps the workspace");
        for (int j = 0; j < ns; ++j) FRCNN_REQUIRE(!merge_overlap(dst[i], src[j]), "eval_merge: a destination buffer overlaps a shard buffer");
        for (int j = i + 1; j < nd; ++j) FRCNN_REQUIRE(!merge_overlap(dst[i], dst[j]), "eval_merge: two destination buffers overlap");
    }
    for (int j = 0; j < ns; ++j) FRCNN_REQUIRE(!merge_overlap(src[j], wsp), "eval_merge: a shard buffer overlaps the workspace");

    const long long tps1 = (SR + MERGE_SCAN_BLOCK - 1) / MERGE_SCAN_BLOCK, tps2 = (SI + MERGE_ROW_BLOCK - 1) / MERGE_ROW_BLOCK;
    ws.NB1 = (long long)W * tps1;                               // <= n1 / MERGE_SCAN_BLOCK + W
    ws.NB2 = (long long)W * tps2;
    const MergeSrc S = {(const int32_t *)sh_score, sh_label, sh_image, sh_order, sh_flags, sh_led_image, (const long long *)sh_led_range, sh_led_delta,
                        (const long long *)sh_n_records, (const long long *)sh_n_images, sh_error, W, (int)SR, (int)SI, (int)counter_words};
    const MergeDst D = {(int32_t *)rec_score, rec_label, rec_image, rec_order, rec_flags, led_image, (long long *)led_range, led_delta,
                        (long long)record_capacity, (long long)image_capacity, (u64 *)counter, (long long *)cursor, (long long *)led_count, error_word,
                        (long long *)snap_cursor, (long long *)snap_counter};
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(MERGE_THREADS);
    long long gi = (ws.TS + MERGE_THREADS - 1) / MERGE_THREADS;
    if (gi > 4096) gi = 4096;
    const unsigned g_occ = (unsigned)((n2 + MERGE_THREADS - 1) / MERGE_THREADS), g_words = (unsigned)((counter_words + MERGE_THREADS - 1) / MERGE_THREADS);
    FRCNN_LAUNCH(merge_init_kernel, dim3((unsigned)gi), blk, 0, s, ws.table, ws.TS, (u64 *)counter, (int)counter_words);
    FRCNN_CHECK_LAUNCH("merge_init_kernel");
    if (n2 > 0) {
        FRCNN_LAUNCH(merge_insert_kernel, dim3(g_occ), blk, 0, s, S, ws.table, ws.TS);
        FRCNN_CHECK_LAUNCH("merge_insert_kernel");
        FRCNN_LAUNCH(merge_keep_kernel, dim3((unsigned)ws.NB2), blk, 0, s, S, (const u64 *)ws.table, ws.TS, ws.keep_row, ws.lb_cnt, ws.lb_len);
        FRCNN_CHECK_LAUNCH("merge_keep_kernel");
    }
    if (n1 > 0) {
        FRCNN_LAUNCH(merge_flag_kernel, dim3((unsigned)ws.NB1), blk, 0, s, S, (const uint8_t *)ws.keep_row, ws.keep_rec, ws.rb);
        FRCNN_CHECK_LAUNCH("merge_flag_kernel");
    }
    FRCNN_LAUNCH(merge_scan_kernel, dim3(1), blk, 0, s, S, D, ws.rb, ws.NB1, ws.lb_cnt, ws.lb_len, ws.NB2);
    FRCNN_CHECK_LAUNCH("merge_scan_kernel");
    if (n1 > 0) {
        if (flags_width == 4)
            FRCNN_LAUNCH(merge_scatter_kernel<4>, dim3((unsigned)ws.NB1), blk, 0, s, S, D, (const uint8_t *)ws.keep_rec, (const u64 *)ws.rb);
        else
            FRCNN_LAUNCH(merge_scatter_kernel<1>, dim3((unsigned)ws.NB1), blk, 0, s, S, D, (const uint8_t *)ws.keep_rec, (const u64 *)ws.rb);
        FRCNN_CHECK_LAUNCH("merge_scatter_kernel");
    }
    if (n2 > 0) {
        FRCNN_LAUNCH(merge_ledger_kernel, dim3((unsigned)ws.NB2), blk, 0, s, S, D, (const uint8_t *)ws.keep_row, (const u64 *)ws.lb_cnt,
                     (const u64 *)ws.lb_len);
        FRCNN_CHECK_LAUNCH("merge_ledger_kernel");
    }
    FRCNN_LAUNCH(merge_finish_kernel, dim3(g_words), blk, 0, s, (const u64 *)counter, (long long *)snap_counter, (int)counter_words);
    FRCNN_CHECK_LAUNCH("merge_finish_kernel");
    return FRCNN_OK;
}
