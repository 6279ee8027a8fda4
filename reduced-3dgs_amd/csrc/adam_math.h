// adam_math.h -- per-element arithmetic of the fused Adam step (optim.hip), shared with the CPU test shim
// tests/hostcheck_optim/hostcheck_optim.hip so the exact source the kernel executes per lane is checked without a GPU.
//
// It reproduces torch.optim.Adam's default (foreach) step for fp32 tensors with amsgrad, maximize, weight_decay and
// capturable all off, op for op and rounding for rounding.  That step is five elementwise passes per tensor list:
//   m <- lerp(m, g, 1 - beta1)
//   v <- v * beta2
//   v <- addcmul(v, g, g, value = 1 - beta2)
//   d <- sqrt(v) / bc2_sqrt + eps
//   p <- addcdiv(p, m, d, value = step_size)
// with host scalars computed in Python doubles (step: the count after this step's bump)
//   bc1 = 1 - beta1**step,  bc2 = 1 - beta2**step,  step_size = -(lr / bc1),  bc2_sqrt = bc2**0.5
// and each rounded to fp32 once on its way into the kernel, as are 1 - beta1, beta2, 1 - beta2 and eps (AdamScalars).
//
// Where torch's ROCm build rounds was settled on an MI355X against torch 2.10 (ROCm 7.0) on the same inputs, one sweep
// over the sixteen variants {lerp, addcmul, addcdiv: one fma or a rounded product and sum} x {divide by bc2_sqrt or
// multiply by its reciprocal}: only the variant written here reproduces torch's p, m and v bit for bit.
// Each line below names its roundings.  optim.hip is compiled with -ffp-contract=off and correctly rounded fp32 divide
// and sqrt, so the compiler adds and removes none: the fmas are explicit (__fmaf_rn on the device, fmaf on the host).
#ifndef R3DGS_ADAM_MATH_H
#define R3DGS_ADAM_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

// The fp32 scalars of one tensor's step.  Each is a double of the host (or of the capturable kernel) rounded once.
struct AdamScalars {
    float w1;          // 1 - beta1, the lerp weight
    float beta2;
    float w2;          // 1 - beta2, the addcmul value
    float bc2_sqrt;    // (1 - beta2**step) ** 0.5
    float eps;
    float step_size;   // -(lr / (1 - beta1**step))
};

__host__ __device__ inline float adam_fma(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return std::fma(a, b, c);
#endif
}

// One element: updates p, m, v in place.
__host__ __device__ inline void adam_element(const AdamScalars& s, float g, float& p, float& m, float& v)
{
    // lerp(m, g, w1) -- torch takes the form with the smaller weight: m + w1 (g - m) for w1 < 0.5, else
    // g - (g - m)(1 - w1); the difference and (1 - w1) rounded, then one fma
    const float dg = g - m;                                                              // 1 rounding
    m = s.w1 < 0.5f ? adam_fma(s.w1, dg, m)                                              // 1 rounding (fma)
                    : adam_fma(-dg, 1.0f - s.w1, g);                                     // 2 roundings (1 - w1, fma)
    v = v * s.beta2;                                                                     // 1 rounding
    v = adam_fma(s.w2, g * g, v);                                                        // 2 roundings (g g, fma)
    const float d = std::sqrt(v) / s.bc2_sqrt + s.eps;                                   // 3 roundings (sqrt, /, +)
    p = adam_fma(s.step_size, m / d, p);                                                 // 2 roundings (m / d, fma)
}

}  // namespace r3

#endif  // R3DGS_ADAM_MATH_H
