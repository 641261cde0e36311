// sgd_dev.h -- the multi-tensor table of the optimizer (built in sgd.hip), shared by layout between sgd.hip (the update), grad_norm.hip
// (the gradient norm in front of it) and telemetry.hip (the per-tensor statistics); grad_accum.hip takes the two constants.  The code these
// files share -- chunk lookup, sweep, host-side checks -- is multi_tensor_dev.h's, the chunk body of the sums of squares sumsq_dev.h's.
//   SgdHeader | SgdRow[n_tensors] {parameter, gradient, momentum, numel, group, vec} | int2 map[n_chunks] {tensor, chunk in tensor}
// One workgroup of SGD_THREADS threads per map entry, SGD_CHUNK elements of one tensor.  Sizes, offsets and the two constants are part of
// the layout stamp (frcnn_layout.h).
#pragma once
#include "frcnn_common.h"

#define SGD_CHUNK 8192                  // elements per workgroup: 256 threads x 8 float4
#define SGD_THREADS 256
#define SGD_MAGIC 0x31444753u           // "SGD1"
#define SGD_MAX_TENSORS 65536
#define SGD_MAX_GROUPS 1024

typedef float sgd_f4 __attribute__((ext_vector_type(4)));
struct SgdHeader { uint32_t magic; int32_t n_tensors, n_groups, n_chunks, chunk, pad[3]; uint64_t rows_off, map_off, bytes, pad2; };
struct SgdRow { float *p; const float *g; float *m; int64_t numel; int32_t group, vec, pad[2]; };
static_assert(sizeof(SgdHeader) == 64 && sizeof(SgdRow) == 48, "sgd table layout");
static_assert(SGD_CHUNK % (4 * SGD_THREADS) == 0, "a chunk is a whole number of float4 sweeps");

static inline size_t sgd_table_bytes(int64_t n_tensors, int64_t n_chunks)
{
    return sizeof(SgdHeader) + (size_t)n_tensors * sizeof(SgdRow) + (size_t)n_chunks * sizeof(int2);
}
