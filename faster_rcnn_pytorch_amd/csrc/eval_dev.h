// eval_dev.h -- what the two evaluator translation units (eval.hip: the VOC protocol, coco_eval.hip: the COCO protocol) share: the bits
// of the device error word and the order of fp32 scores as unsigned integers.
#pragma once
#include "frcnn_common.h"

// device error word (evaluation.py reports them)
#define EVAL_ERR_UPSTREAM_ABORT 1      // count < 0: an aborted proposal scan upstream
#define EVAL_ERR_GT_OVERFLOW 2         // n_gt > the ground-truth capacity
#define EVAL_ERR_COUNT_RANGE 4         // count > the detection capacity
#define EVAL_ERR_LABEL_RANGE 8         // a label outside 0 .. C-2

typedef unsigned long long u64;

#ifdef __HIPCC__
// monotone in the float's value; -0 folded onto +0 (Python's sort sees them as equal)
__device__ __forceinline__ uint32_t eval_orderable(float score)
{
    const uint32_t u = __float_as_uint(score == 0.0f ? 0.0f : score);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
#endif
