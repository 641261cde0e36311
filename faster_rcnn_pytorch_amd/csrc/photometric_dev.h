// photometric_dev.h -- the per-pixel arithmetic of csrc/photometric.hip: Pillow's Image.blend, convert("L"), convert("HSV") and
// convert("RGB") from HSV, operation for operation and in Pillow's number formats (include/frcnn_hip.h lists the forms;
// tests/photometric_ref.py restates them in numpy).  Needs -ffp-contract=off (the blend is a multiply, a rounding, then an add) and a
// correctly rounded binary32 division (hipcc's default).  Plain C++ apart from PM_HD, so the same text can be compiled for the host.
#pragma once
#include <stdint.h>
#include <math.h>

#ifdef __HIPCC__
#define PM_HD __host__ __device__ __forceinline__
#else
#define PM_HD static inline
#endif

enum { PM_BRIGHTNESS = 0, PM_CONTRAST = 1, PM_SATURATION = 2, PM_HUE = 3 };

struct PmPixel { uint32_t r, g, b; };

// the plan as the kernels use it: the live slots in order (an op outside 0..3 and an op's second appearance are dropped).  No arrays:
// the plan is the same for every lane, and with named fields it stays in scalar registers.
struct PmPlan {
    int n, contrast_at;                   // live slots; the slot that holds contrast, or -1
    uint32_t ops;                         // 4 bits per live slot
    uint32_t p0, p1, p2, p3;              // the slots' parameters
};
PM_HD int pm_op(const PmPlan &P, int k) { return (int)((P.ops >> (4 * k)) & 15u); }
PM_HD uint32_t pm_param(const PmPlan &P, int k) { return k == 0 ? P.p0 : (k == 1 ? P.p1 : (k == 2 ? P.p2 : P.p3)); }

PM_HD PmPlan pm_decode(const int32_t *plan)
{
    PmPlan P;
    P.n = 0; P.contrast_at = -1; P.ops = 0; P.p0 = P.p1 = P.p2 = P.p3 = 0;
    uint32_t seen = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = plan[2 * k];
        const uint32_t param = (uint32_t)plan[2 * k + 1];
        if (op < 0 || op > 3 || ((seen >> op) & 1u)) continue;
        seen |= 1u << op;
        if (op == PM_CONTRAST) P.contrast_at = P.n;
        P.ops |= (uint32_t)op << (4 * P.n);
        if (P.n == 0) P.p0 = param; else if (P.n == 1) P.p1 = param; else if (P.n == 2) P.p2 = param; else P.p3 = param;
        ++P.n;
    }
    return P;
}

PM_HD float pm_bits_to_float(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }

PM_HD uint32_t pm_luma(PmPixel p) { return (19595u * p.r + 38470u * p.g + 7471u * p.b + 0x8000u) >> 16; }

// Image.blend(degenerate a, image b, alpha) for one byte
PM_HD uint32_t pm_blend(uint32_t a, uint32_t b, float alpha)
{
    const float fa = (float)(int)a;
    const float prod = alpha * (float)((int)b - (int)a);
    const float t = fa + prod;
    if (alpha >= 0.0f && alpha <= 1.0f) return (uint32_t)(int)t & 255u;
    return t <= 0.0f ? 0u : (t >= 255.0f ? 255u : (uint32_t)(int)t);
}

PM_HD uint32_t pm_clip8(int v) { return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v); }
PM_HD uint32_t pm_round8(double v) { return pm_clip8((int)round(v)); }

// convert("HSV"), H += shift (mod 256), convert("RGB")
PM_HD PmPixel pm_hue(PmPixel p, uint32_t shift)
{
    const uint32_t mx = p.r > p.g ? (p.r > p.b ? p.r : p.b) : (p.g > p.b ? p.g : p.b);
    const uint32_t mn = p.r < p.g ? (p.r < p.b ? p.r : p.b) : (p.g < p.b ? p.g : p.b);
    uint32_t H = 0, S = 0;
    const uint32_t V = mx;
    if (mx != mn) {
        const float cr = (float)(int)(mx - mn);
        const float s = cr / (float)(int)mx;
        const float rc = (float)(int)(mx - p.r) / cr, gc = (float)(int)(mx - p.g) / cr, bc = (float)(int)(mx - p.b) / cr;
        float h;
        if (p.r == mx) h = bc - gc;
        else if (p.g == mx) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        double x = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6]: fmod(x, 1.0) is x - floor(x), exactly
        x = x - floor(x);
        h = (float)x;
        H = pm_clip8((int)((double)h * 255.0));
        S = pm_clip8((int)((double)s * 255.0));
    }
    H = (H + shift) & 255u;
    PmPixel o;
    if (S == 0) { o.r = o.g = o.b = V; return o; }
    const double x = (double)(int)H * 6.0 / 255.0;
    const double fl = floor(x);
    const double f = (double)(float)(x - fl);
    const double fs = (double)(float)((double)(int)S / 255.0);
    const double v = (double)(int)V;
    const uint32_t pp = pm_round8(v * (1.0 - fs)), q = pm_round8(v * (1.0 - fs * f)), t = pm_round8(v * (1.0 - fs * (1.0 - f)));
    switch ((int)fl % 6) {
    case 0: o.r = V; o.g = t; o.b = pp; break;
    case 1: o.r = q; o.g = V; o.b = pp; break;
    case 2: o.r = pp; o.g = V; o.b = t; break;
    case 3: o.r = pp; o.g = q; o.b = V; break;
    case 4: o.r = t; o.g = pp; o.b = V; break;
    default: o.r = V; o.g = pp; o.b = q; break;
    }
    return o;
}

// the live slots [lo, hi) of a plan on one pixel; mean: the contrast degenerate (read only when contrast lies in the range)
PM_HD PmPixel pm_apply(const PmPlan &P, int lo, int hi, uint32_t mean, PmPixel p)
{
    for (int k = lo; k < hi; ++k) {
        const int op = pm_op(P, k);
        if (op == PM_HUE) { p = pm_hue(p, pm_param(P, k) & 255u); continue; }
        const float alpha = pm_bits_to_float(pm_param(P, k));
        uint32_t dr = 0, dg = 0, db = 0;
        if (op == PM_CONTRAST) dr = dg = db = mean;
        else if (op == PM_SATURATION) dr = dg = db = pm_luma(p);
        p.r = pm_blend(dr, p.r, alpha); p.g = pm_blend(dg, p.g, alpha); p.b = pm_blend(db, p.b, alpha);
    }
    return p;
}

// int(sum / count + 0.5) in float64: ImageEnhance.Contrast's degenerate level
PM_HD uint32_t pm_mean_level(uint64_t sum, uint64_t count) { return (uint32_t)(int)((double)sum / (double)count + 0.5); }

// four pixels <-> the three dwords that hold them
PM_HD void pm_unpack4(uint32_t w0, uint32_t w1, uint32_t w2, PmPixel px[4])
{
    px[0].r = w0 & 255u; px[0].g = (w0 >> 8) & 255u; px[0].b = (w0 >> 16) & 255u;
    px[1].r = w0 >> 24; px[1].g = w1 & 255u; px[1].b = (w1 >> 8) & 255u;
    px[2].r = (w1 >> 16) & 255u; px[2].g = w1 >> 24; px[2].b = w2 & 255u;
    px[3].r = (w2 >> 8) & 255u; px[3].g = (w2 >> 16) & 255u; px[3].b = w2 >> 24;
}
PM_HD void pm_pack4(const PmPixel px[4], uint32_t *w0, uint32_t *w1, uint32_t *w2)
{
    *w0 = px[0].r | (px[0].g << 8) | (px[0].b << 16) | (px[1].r << 24);
    *w1 = px[1].g | (px[1].b << 8) | (px[2].r << 16) | (px[2].g << 24);
    *w2 = px[2].b | (px[3].r << 8) | (px[3].g << 16) | (px[3].b << 24);
}
