// metrics_math.h -- per-sample arithmetic of the evaluation metrics (metrics.hip), shared with the CPU test shim
// tests/hostcheck_metrics/hostcheck_metrics.hip so the exact source the kernels execute per lane is checked without a GPU.
//
// Reference: train.py:253-265 (clamp both images, l1_loss, psnr) and render.py + metrics.py:24-86 (the render is written
// as an 8-bit PNG by torchvision's save_image, read back with to_tensor, compared with psnr and ssim).
//
// metrics_load turns one stored sample into the fp32 value the reference would have compared:
//   * a float sample as it is; a uint8 sample as float(u) / 255.0f, one correctly rounded fp32 divide (to_tensor);
//   * clamp mode: min(max(x, 0), 1) with torch.clamp's NaN behaviour (NaN stays NaN);
//   * quantise mode: metrics_quantise8(x) / 255.0f, the value metrics.py reads back from the PNG render.py wrote.
// metrics_quantise8 is save_image's x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) with the same fp32 roundings in the same
// order: the product rounded to fp32, the sum rounded to fp32, clamp, truncate.  No FMA may fuse the first two steps: the
// unit is compiled with -ffp-contract=off (build.py EXACT) and the function switches contraction off itself as well.
// NaN maps to 0: the reference leaves that case undefined (a float NaN converted to uint8).
//
// Error terms are taken in double: the difference of two fp32 values is exact in double, so |x - y| is exact and (x - y)^2
// is rounded once at 2^-53.
#ifndef R3DGS_METRICS_MATH_H
#define R3DGS_METRICS_MATH_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace r3 {

constexpr int kMetricsClamp = 1;      // R3DGS_METRICS_CLAMP
constexpr int kMetricsQuantise8 = 2;  // R3DGS_METRICS_QUANTISE8

__host__ __device__ inline uint8_t metrics_quantise8(float x)
{
#pragma clang fp contract(off)
    const float p = x * 255.0f;
    const float s = p + 0.5f;
    if (!(s > 0.0f)) return 0;   // negatives, -0, -inf and NaN
    if (s >= 255.0f) return 255;
    return (uint8_t)s;           // truncation
}

__host__ __device__ inline float metrics_clamp01(float x)
{
    return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);   // NaN compares false twice and stays
}

__host__ __device__ inline float metrics_from_u8(uint8_t u) { return (float)u / 255.0f; }

__host__ __device__ inline float metrics_load(float x, int flags)
{
    if (flags & kMetricsQuantise8) return metrics_from_u8(metrics_quantise8(x));
    return (flags & kMetricsClamp) ? metrics_clamp01(x) : x;
}

// a uint8 sample: already in [0, 1] and already 8-bit, so neither flag changes it
__host__ __device__ inline float metrics_load(uint8_t u, int) { return metrics_from_u8(u); }

__host__ __device__ inline double metrics_abs_err(float x, float y)
{
    const double d = (double)x - (double)y;
    return d < 0.0 ? -d : d;   // NaN stays NaN
}

__host__ __device__ inline double metrics_sq_err(float x, float y)
{
    const double d = (double)x - (double)y;
    return d * d;
}

}  // namespace r3

#endif  // R3DGS_METRICS_MATH_H
