// stats_math.h -- per-element arithmetic of the per-iteration training statistics (train_stats.hip), shared with the CPU
// test shim tests/hostcheck_stats/hostcheck_stats.hip so the exact source the kernels execute per lane is checked without a GPU.
//
// What it restates (the reference's loop around loss.backward()):
//   train.py:105-106            Lalpha_regul = get_opacity[visibility_filter].abs().mean()       stats_sigmoid, per visible lane
//   (autograd of the line above) d sigmoid / d opacity, scaled by upstream / n_visible            stats_sigmoid_grad, alpha_regul_term
//   train.py:134                max_radii2D[vis] = max(max_radii2D[vis], radii[vis])             densify_update
//   gaussian_model.py:693-695   xyz_gradient_accum += ||viewspace.grad[:, :2]||;  denom += vis   densify_update
// train_stats.hip is compiled with -ffp-contract=off and correctly rounded fp32 divide and sqrt (build.py EXACT), so the
// roundings named below are the ones executed, on the device as on the host.
#ifndef R3DGS_STATS_MATH_H
#define R3DGS_STATS_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

// The opacity activation, written once: 1 / (1 + exp(-x)).  Roundings: expf (<= 1 ulp), the add, the divide.
__host__ __device__ inline float stats_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// d sigmoid(x) / dx = s (1 - s), evaluated as t / (1 + t)^2 with t = exp(-|x|) (the derivative is even in x).  The product
// s (1 - s) itself cancels in 1 - s once s is near 1 (x = 10: three digits are left); this form has no subtraction and t <= 1
// cannot overflow.  Roundings: expf (<= 1 ulp), the add (its error enters twice), the multiply, the divide.
__host__ __device__ inline float stats_sigmoid_grad(float x)
{
    const float t = expf(-fabsf(x));
    const float d = 1.f + t;
    return t / (d * d);
}

// One element of alpha_regul_backward: the addend of dL_dopacity[i] for a visible Gaussian, `scale` = upstream / n_visible
// (one divide per thread, train_stats.hip).  Roundings: stats_sigmoid_grad's, then the multiply.
__host__ __device__ inline float alpha_regul_term(float x, float scale) { return stats_sigmoid_grad(x) * scale; }

// One Gaussian of densification_stats, in place.  gx, gy: viewspace_grad[i, 0:2] (ignored when the Gaussian is culled).
// Roundings: the two squares, their sum, the square root (the same expression as pack_view_stats_kernel), the add into the
// accumulator; denom counts in fp32 as the reference's tensor does; (float)radii is exact below 2^24.
__host__ __device__ inline void densify_update(int radii, float gx, float gy, float& grad_accum, float& denom, float& max_radii)
{
    const bool vis = radii > 0;
    grad_accum = grad_accum + (vis ? sqrtf(gx * gx + gy * gy) : 0.f);
    denom = denom + (vis ? 1.f : 0.f);
    max_radii = vis ? fmaxf(max_radii, (float)radii) : max_radii;
}

}  // namespace r3

#endif  // R3DGS_STATS_MATH_H
