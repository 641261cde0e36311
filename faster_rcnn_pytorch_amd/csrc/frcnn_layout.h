// frcnn_layout.h -- the layout stamp: one 64-bit value computed AT COMPILE TIME in every translation unit from the sizes, field offsets
// and constants of everything the translation units of this library share by layout rather than through a function call:
//   * AnchorDesc        (frcnn_internal.h): filled on the host in boxes.hip, handed by value to kernels of boxes.hip / proposal.hip;
//   * SsCtl + ss_plan() (topk_dev.h): the sample sort's control block and its (samples, stride) plan -- WRITTEN by the proposal
//     prologue's sampling workgroups (boxes.hip) and READ by topk_partition / topk_bucket (topk.hip), each from its own copy of the
//     header: two objects compiled against two versions of it disagree about where the splitters, counts and barrier words lie and
//     how large a bucket can get (round 3, 14:49: DESIGN.md section 7);
//   * SgdHeader / SgdRow + SGD_CHUNK / SGD_THREADS (sgd_dev.h): the optimizer's table, BUILT in sgd.hip and walked by the kernels of sgd.hip,
//     grad_norm.hip and telemetry.hip, each through multi_tensor_dev.h's chunk lookup (that header holds code, no layout: nothing of it is
//     stamped); frcnn_grad_norm_state (include/frcnn_hip.h): written by grad_norm.hip, its coef and skip words read by sgd.hip's
//     kernels through pointers the caller derives from the same struct; frcnn_grad_accum_state (include/frcnn_hip.h): written by
//     grad_accum.hip, its hold word read by the same kernels as their skip word or user guard;
//   * EmaHeader / EmaRow (ema_dev.h): the weight average's table, BUILT in ema.hip and walked by the kernels of ema.hip and by sgd.hip's
//     fused update; frcnn_ema_state (include/frcnn_hip.h): written by ema.hip's advance and swap kernels, its w and swapped words read by
//     sgd.hip's kernels;
//   * frcnn_tensor_stats_row / _state and frcnn_journal_totals / _state (include/frcnn_hip.h): written by telemetry.hip, read by the caller
//     (telemetry.py) by offset;
//   * DmArgs / DmWs + the DM_* limits (detect_merge_dev.h): the merge's kernel-argument rows and workspace carving, FILLED by dm_prepare in
//     detect_merge.hip and read by the class kernels of detect_merge.hip and detect_soft.hip, whose rows the emit kernel of detect_merge.hip
//     then reads back from the workspace;
//   * the profiling table size and the ABI version.
// Every object registers its stamp in a static initialiser; frcnn_layout_check() (api.cpp; also run by frcnn_abi_version()) compares
// them all with api.cpp's own and names the object that disagrees -- the library then refuses to load (FRCNN_ERR_UNSUPPORTED) instead of
// running kernels against a foreign layout.  A header edit that is not followed by a rebuild of every dependent object is therefore an
// import error, not an out-of-bounds access.  (The Makefile also makes every object depend on every header and on compiler-generated
// dependency files; the stamp is the check that does not rely on the build system.)
#pragma once
#include <cstddef>
#include "frcnn_internal.h"
#include "topk_dev.h"
#include "sgd_dev.h"
#include "ema_dev.h"
#include "detect_merge_dev.h"

constexpr uint64_t frcnn_lay_mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }

constexpr uint64_t frcnn_lay_plan(uint64_t h, int64_t N, int64_t K)
{
    int S = 0, stride = 0;
    ss_plan(N, K, &S, &stride);
    return frcnn_lay_mix(frcnn_lay_mix(h, (uint64_t)S), (uint64_t)stride);
}

constexpr uint64_t frcnn_layout_stamp_value()
{
    uint64_t h = 0xcbf29ce484222325ull;
#define LAY(v) h = frcnn_lay_mix(h, (uint64_t)(v))
    LAY(FRCNN_ABI_VERSION); LAY(FRCNN_PROF_MAX_KERNELS); LAY(FRCNN_MAX_LEVELS); LAY(FRCNN_MAX_BASE);
    LAY(sizeof(AnchorDesc)); LAY(offsetof(AnchorDesc, n_levels)); LAY(offsetof(AnchorDesc, A)); LAY(offsetof(AnchorDesc, fh));
    LAY(offsetof(AnchorDesc, fw)); LAY(offsetof(AnchorDesc, sh)); LAY(offsetof(AnchorDesc, sw)); LAY(offsetof(AnchorDesc, off));
    LAY(offsetof(AnchorDesc, base)); LAY(offsetof(AnchorDesc, div_w)); LAY(offsetof(AnchorDesc, div_h));
    LAY(SS_BUCKETS); LAY(SS_MIN_N); LAY(SS_LARGE);
    LAY(sizeof(SsCtl)); LAY(offsetof(SsCtl, split)); LAY(offsetof(SsCtl, cnt)); LAY(offsetof(SsCtl, cursor)); LAY(offsetof(SsCtl, n_valid));
    LAY(offsetof(SsCtl, pad)); LAY(offsetof(SsCtl, bar)); LAY(offsetof(SsCtl, flag));
    h = frcnn_lay_plan(h, 20646, 12000); h = frcnn_lay_plan(h, 20646, 6000); h = frcnn_lay_plan(h, 268569, 4000);
    h = frcnn_lay_plan(h, 268569, 2000); h = frcnn_lay_plan(h, 65536, 65536); h = frcnn_lay_plan(h, 4096, 300);
    LAY(SGD_CHUNK); LAY(SGD_THREADS); LAY(sizeof(SgdHeader)); LAY(sizeof(SgdRow)); LAY(offsetof(SgdRow, p)); LAY(offsetof(SgdRow, g));
    LAY(offsetof(SgdRow, m)); LAY(offsetof(SgdRow, numel)); LAY(offsetof(SgdRow, group)); LAY(offsetof(SgdRow, vec));
    LAY(sizeof(frcnn_grad_norm_state)); LAY(offsetof(frcnn_grad_norm_state, max_norm)); LAY(offsetof(frcnn_grad_norm_state, flags));
    LAY(offsetof(frcnn_grad_norm_state, sumsq)); LAY(offsetof(frcnn_grad_norm_state, norm)); LAY(offsetof(frcnn_grad_norm_state, coef));
    LAY(offsetof(frcnn_grad_norm_state, skip)); LAY(offsetof(frcnn_grad_norm_state, nonfinite)); LAY(offsetof(frcnn_grad_norm_state, steps));
    LAY(offsetof(frcnn_grad_norm_state, skipped_steps)); LAY(FRCNN_GRAD_NORM_FINISH_THREADS);
    LAY(sizeof(frcnn_grad_accum_state)); LAY(offsetof(frcnn_grad_accum_state, window)); LAY(offsetof(frcnn_grad_accum_state, phase));
    LAY(offsetof(frcnn_grad_accum_state, live)); LAY(offsetof(frcnn_grad_accum_state, hold)); LAY(offsetof(frcnn_grad_accum_state, windows));
    LAY(offsetof(frcnn_grad_accum_state, frames)); LAY(offsetof(frcnn_grad_accum_state, dropped)); LAY(FRCNN_GRAD_ACCUM_ROWS);
    LAY(sizeof(EmaHeader)); LAY(sizeof(EmaRow)); LAY(offsetof(EmaRow, p)); LAY(offsetof(EmaRow, e)); LAY(offsetof(EmaRow, numel)); LAY(offsetof(EmaRow, vec));
    LAY(sizeof(frcnn_ema_state)); LAY(offsetof(frcnn_ema_state, decay)); LAY(offsetof(frcnn_ema_state, num_updates)); LAY(offsetof(frcnn_ema_state, w));
    LAY(offsetof(frcnn_ema_state, flags)); LAY(offsetof(frcnn_ema_state, swapped)); LAY(offsetof(frcnn_ema_state, skipped));
    LAY(offsetof(frcnn_ema_state, refused));
    LAY(sizeof(frcnn_tensor_stats_row)); LAY(offsetof(frcnn_tensor_stats_row, g_sumsq)); LAY(offsetof(frcnn_tensor_stats_row, p_sumsq));
    LAY(offsetof(frcnn_tensor_stats_row, m_sumsq)); LAY(offsetof(frcnn_tensor_stats_row, g_absmax)); LAY(offsetof(frcnn_tensor_stats_row, p_absmax));
    LAY(offsetof(frcnn_tensor_stats_row, g_nonfinite)); LAY(offsetof(frcnn_tensor_stats_row, p_nonfinite)); LAY(offsetof(frcnn_tensor_stats_row, m_read));
    LAY(sizeof(frcnn_tensor_stats_state)); LAY(offsetof(frcnn_tensor_stats_state, every)); LAY(offsetof(frcnn_tensor_stats_state, tick));
    LAY(offsetof(frcnn_tensor_stats_state, measured_tick)); LAY(offsetof(frcnn_tensor_stats_state, measures));
    LAY(offsetof(frcnn_tensor_stats_state, first_nonfinite_g)); LAY(offsetof(frcnn_tensor_stats_state, first_nonfinite_p));
    LAY(FRCNN_TENSOR_STATS_FINISH_THREADS); LAY(sizeof(frcnn_journal_totals)); LAY(sizeof(frcnn_journal_state)); LAY(FRCNN_JOURNAL_MAX_COLS);
    LAY(sizeof(DmArgs)); LAY(offsetof(DmArgs, labels)); LAY(offsetof(DmArgs, scores)); LAY(offsetof(DmArgs, counts)); LAY(offsetof(DmArgs, caps));
    LAY(offsetof(DmArgs, flags)); LAY(offsetof(DmArgs, K)); LAY(sizeof(DmWs)); LAY(DM_MAX_K); LAY(DM_MAX_CAND); LAY(DM_THREADS); LAY(DM_ROW_BITS);
#ifdef FRCNN_LAYOUT_TEST_SKEW          // tests/test_cabi.py builds ONE object with this defined and expects the library to refuse to load
    LAY(FRCNN_LAYOUT_TEST_SKEW);
#endif
#undef LAY
    return h;
}

// the structs as this revision lays them out (a deliberate change updates these lines together with the struct)
static_assert(sizeof(SsCtl) == 8 * SS_BUCKETS + 4 * SS_BUCKETS + 4 * SS_BUCKETS + 64 + 18 * 64 + 64, "SsCtl: unexpected size");
static_assert(offsetof(SsCtl, cnt) == 8 * SS_BUCKETS && offsetof(SsCtl, cursor) == 12 * SS_BUCKETS && offsetof(SsCtl, n_valid) == 16 * SS_BUCKETS,
              "SsCtl: split / cnt / cursor / n_valid moved");
static_assert(offsetof(SsCtl, bar) % 64 == 0 && offsetof(SsCtl, flag) % 64 == 0, "SsCtl: the barrier lines must stay 64-byte aligned");
static_assert(sizeof(AnchorDesc) == 8 + 4 * 4 * FRCNN_MAX_LEVELS + 8 * FRCNN_MAX_LEVELS + 16 * FRCNN_MAX_LEVELS * FRCNN_MAX_BASE + 8,
              "AnchorDesc: unexpected size (kernarg struct of the prologue / anchor kernels)");
static_assert(sizeof(AnchorDesc) <= 4096, "AnchorDesc must fit the kernarg segment");
static_assert(sizeof(frcnn_grad_norm_state) == 64 && offsetof(frcnn_grad_norm_state, sumsq) == 8 && offsetof(frcnn_grad_norm_state, norm) == 16 &&
                  offsetof(frcnn_grad_norm_state, coef) == 20 && offsetof(frcnn_grad_norm_state, skip) == 24 &&
                  offsetof(frcnn_grad_norm_state, nonfinite) == 28 && offsetof(frcnn_grad_norm_state, steps) == 32 &&
                  offsetof(frcnn_grad_norm_state, skipped_steps) == 36,
              "frcnn_grad_norm_state: the offsets include/frcnn_hip.h documents (optim.py reads the block by them)");
static_assert(sizeof(frcnn_grad_accum_state) == 64 && offsetof(frcnn_grad_accum_state, window) == 0 && offsetof(frcnn_grad_accum_state, phase) == 4 &&
                  offsetof(frcnn_grad_accum_state, live) == 8 && offsetof(frcnn_grad_accum_state, hold) == 12 &&
                  offsetof(frcnn_grad_accum_state, windows) == 16 && offsetof(frcnn_grad_accum_state, frames) == 20 &&
                  offsetof(frcnn_grad_accum_state, dropped) == 24,
              "frcnn_grad_accum_state: the offsets include/frcnn_hip.h documents (optim.py reads the block by them; hold is sgd.hip's skip word)");
static_assert(sizeof(frcnn_ema_state) == 64 && offsetof(frcnn_ema_state, decay) == 0 && offsetof(frcnn_ema_state, num_updates) == 8 &&
                  offsetof(frcnn_ema_state, w) == 16 && offsetof(frcnn_ema_state, flags) == 20 && offsetof(frcnn_ema_state, swapped) == 24 &&
                  offsetof(frcnn_ema_state, skipped) == 28 && offsetof(frcnn_ema_state, refused) == 32,
              "frcnn_ema_state: the offsets include/frcnn_hip.h documents (optim.py reads and writes the block by them)");
static_assert(sizeof(frcnn_tensor_stats_row) == 64 && offsetof(frcnn_tensor_stats_row, p_sumsq) == 8 && offsetof(frcnn_tensor_stats_row, m_sumsq) == 16 &&
                  offsetof(frcnn_tensor_stats_row, g_absmax) == 24 && offsetof(frcnn_tensor_stats_row, p_absmax) == 28 &&
                  offsetof(frcnn_tensor_stats_row, g_nonfinite) == 32 && offsetof(frcnn_tensor_stats_row, p_nonfinite) == 36 &&
                  offsetof(frcnn_tensor_stats_row, m_read) == 40,
              "frcnn_tensor_stats_row: the offsets include/frcnn_hip.h documents (telemetry.py reads the rows by them)");
static_assert(sizeof(frcnn_tensor_stats_state) == 64 && offsetof(frcnn_tensor_stats_state, every) == 0 && offsetof(frcnn_tensor_stats_state, tick) == 4 &&
                  offsetof(frcnn_tensor_stats_state, measured_tick) == 8 && offsetof(frcnn_tensor_stats_state, measures) == 12 &&
                  offsetof(frcnn_tensor_stats_state, first_nonfinite_g) == 16 && offsetof(frcnn_tensor_stats_state, first_nonfinite_p) == 20,
              "frcnn_tensor_stats_state: the offsets include/frcnn_hip.h documents (telemetry.py reads and writes the block by them)");
static_assert(sizeof(frcnn_journal_totals) == 40 && offsetof(frcnn_journal_totals, count) == 8 && offsetof(frcnn_journal_totals, max) == 16 &&
                  offsetof(frcnn_journal_totals, min) == 24 && offsetof(frcnn_journal_totals, nonfinite) == 32 && sizeof(frcnn_journal_state) == 64 &&
                  offsetof(frcnn_journal_state, cursor) == 0 && offsetof(frcnn_journal_state, capacity) == 8 && offsetof(frcnn_journal_state, n_cols) == 12,
              "frcnn_journal_totals / frcnn_journal_state: the offsets include/frcnn_hip.h documents (telemetry.py reads and writes them)");

void frcnn_layout_register(const char *object, uint64_t stamp);
int frcnn_layout_check_impl(void);

// one per translation unit, at file scope
#define FRCNN_LAYOUT_STAMP(object) \
    static const int _frcnn_layout_registered_##object = (frcnn_layout_register(#object, frcnn_layout_stamp_value()), 0)
