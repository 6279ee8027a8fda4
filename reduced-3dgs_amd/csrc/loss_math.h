// loss_math.h -- per-pixel arithmetic of the fused L1 + D-SSIM loss (loss.hip), shared with the CPU test shim
// tests/hostcheck_loss/hostcheck_loss.hip so the exact source the kernels execute per lane is checked without a GPU.
//
// Reference: utils/loss_utils.py:33-66 (ssim / _ssim).  From the five filtered moments of one pixel
//   mu_x = F[x], mu_y = F[y], E_xx = F[x*x], E_yy = F[y*y], E_xy = F[x*y]
// (F = the 11x11 Gaussian window, sigma 1.5, zero padding 5) the SSIM value is
//   S = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),
//   s_xx = E_xx - mu_x^2,  s_yy = E_yy - mu_y^2,  s_xy = E_xy - mu_x mu_y.
// With A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_xx + s_yy + C2, D = B1 B2, the partials
// the backward needs (with respect to the three moments that depend on x; mu_y, E_yy are constants) are
//   dS/dmu_x = (2 mu_y (A2 - A1) - 2 mu_x S (B2 - B1)) / D
//   dS/dE_xx = -S B1 / D            (= -S / B2)
//   dS/dE_xy = 2 A1 / D
// written without a division by A1 or A2, which may be 0.  The differences of moments use fma, so E_xx - mu_x^2 is
// rounded once (the product is exact inside the fma): near-zero variances next to large means keep their digits.
#ifndef R3DGS_LOSS_MATH_H
#define R3DGS_LOSS_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

constexpr int kSsimTaps = 11;
constexpr int kSsimRadius = kSsimTaps / 2;
// the reference adds the Python floats 0.01 ** 2 and 0.03 ** 2 to fp32 tensors: the doubles rounded to fp32
constexpr float kSsimC1 = (float)(0.01 * 0.01);
constexpr float kSsimC2 = (float)(0.03 * 0.03);

struct SsimPixel {
    float s;       // SSIM value
    float d_mu;    // dS/dmu_x
    float d_exx;   // dS/dE_xx
    float d_exy;   // dS/dE_xy
};

__host__ __device__ inline SsimPixel ssim_pixel(float mx, float my, float exx, float eyy, float exy)
{
    const float sxx = fmaf(-mx, mx, exx), syy = fmaf(-my, my, eyy), sxy = fmaf(-mx, my, exy);
    const float a1 = fmaf(2.f * mx, my, kSsimC1), a2 = 2.f * sxy + kSsimC2;
    const float b1 = fmaf(mx, mx, fmaf(my, my, kSsimC1)), b2 = (sxx + syy) + kSsimC2;
    const float inv = 1.f / (b1 * b2);
    SsimPixel p;
    p.s = (a1 * a2) * inv;
    p.d_mu = (2.f * my * (a2 - a1) - 2.f * mx * p.s * (b2 - b1)) * inv;
    p.d_exx = -p.s * b1 * inv;
    p.d_exy = 2.f * a1 * inv;
    return p;
}

// |x - y| and the derivative of |x - y| with respect to x, torch's convention sign(0) = 0
__host__ __device__ inline float l1_sign(float x, float y)
{
    const float d = x - y;
    return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
}

}  // namespace r3

#endif  // R3DGS_LOSS_MATH_H
