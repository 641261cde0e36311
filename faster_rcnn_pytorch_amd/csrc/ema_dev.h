// ema_dev.h -- the multi-tensor table of the weight average (built in ema.hip), shared by layout between ema.hip (the stand-alone update,
// the swap, the advance) and sgd.hip (the update fused into the optimizer step):
//   EmaHeader | EmaRow[n_tensors] {parameter, shadow, numel, vec} | int2 map[n_chunks] {tensor, chunk in tensor}
// Chunked with SGD_CHUNK / SGD_THREADS: for the same tensor sizes the map is entry for entry the SGD table's map, so the fused kernel
// finds its EMA row under the tensor number of its SGD map entry.  Sizes and offsets are part of the layout stamp (frcnn_layout.h).
// This header keeps the layout and the rule (ema_one); chunk lookup, sweep and the builder's checks are multi_tensor_dev.h's.
#pragma once
#include "frcnn_common.h"
#include "sgd_dev.h"

#define EMA_MAGIC 0x31414d45u           // "EMA1"

struct EmaHeader { uint32_t magic; int32_t n_tensors, n_chunks, chunk, pad[4]; uint64_t rows_off, map_off, bytes, pad2; };
struct EmaRow { float *p; float *e; int64_t numel; int32_t vec, pad; };
static_assert(sizeof(EmaHeader) == 64 && sizeof(EmaRow) == 32, "ema table layout");

static inline size_t ema_table_bytes(int64_t n_tensors, int64_t n_chunks)
{
    return sizeof(EmaHeader) + (size_t)n_tensors * sizeof(EmaRow) + (size_t)n_chunks * sizeof(int2);
}

// The one-thread bookkeeping launch behind an update (ema.hip): sgd.hip's fused step puts it behind its own two launches.
int ema_advance_launch(frcnn_ema_state *state, const int32_t *skip, hipStream_t stream);

#ifdef __HIPCC__
// torch._foreach_lerp_([e], [p], w) on the CPU, operation for operation: d = round(p - e); |w| < 0.5 ? fma(w, d, e) : fma(round(w - 1), d, p).
// small = |w| < 0.5 and wm1 = round(w - 1) are computed once per workgroup.
__device__ __forceinline__ float ema_one(float p, float e, float w, float wm1, bool small)
{
    const float d = __fsub_rn(p, e);
    return small ? __fmaf_rn(w, d, e) : __fmaf_rn(wm1, d, p);
}
#endif
