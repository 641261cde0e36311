// nms_dev.h -- the IoU suppression decision shared by the NMS kernels (nms.hip) and the fused detection post-process (detect.hip),
// so that both decide every pair with the same instructions.
#pragma once
#include "frcnn_common.h"

#ifdef __HIPCC__
// v_max_f32 / v_min_f32 without LLVM's sNaN-canonicalising v_max(x,x) in front of every operand
__device__ __forceinline__ float vmaxf(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vminf(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// exact form: torchvision's expression, IEEE division (symmetric in its two boxes: fp + and min/max commute)
__device__ __forceinline__ bool nms_suppress_exact(float4 a, float area_a, float4 b, float area_b, float thr)
{
    const float w = vmaxf(vminf(a.z, b.z) - vmaxf(a.x, b.x), 0.0f);
    const float h = vmaxf(vminf(a.w, b.w) - vmaxf(a.y, b.y), 0.0f);
    const float inter = w * h;
    return inter / (area_a + area_b - inter) > thr;
}

// the quotient nms_suppress_exact compares, by the same instructions: for a caller that tests it another way (detect_merge.hip's voters, >=)
__device__ __forceinline__ float nms_iou_exact(float4 a, float area_a, float4 b, float area_b)
{
    const float w = vmaxf(vminf(a.z, b.z) - vmaxf(a.x, b.x), 0.0f);
    const float h = vmaxf(vminf(a.w, b.w) - vmaxf(a.y, b.y), 0.0f);
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}
#endif  // __HIPCC__
