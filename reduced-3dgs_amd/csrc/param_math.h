// param_math.h -- the activations between the model's raw parameters and the rasterizer, and their backward, per element
// with every fp32 rounding written down.  Shared by the per-Gaussian kernels (preprocess.hip, preprocess_bwd.hip), by
// r3dgs_activate_params (capi.hip -> preprocess.hip) and by the CPU test shim tests/hostcheck_params/hostcheck_params.hip,
// so the exact source a lane executes is checked without a GPU.
//
// What it restates (scene/gaussian_model.py of the reference: scaling_activation = torch.exp, rotation_activation =
// torch.nn.functional.normalize):
//   scale     s = exp(raw)                                   dL/draw = dL/ds * s
//   rotation  q = raw / max(||raw||_2, 1e-12)                dL/draw = (g - q (q . g)) / n      for n = ||raw|| > 1e-12
//                                                            dL/draw = g / 1e-12                otherwise (torch's clamp_min
//                                                            hands the norm no gradient below the clamp; at n == 1e-12
//                                                            exactly torch takes the first form -- a set of measure zero)
//
// The translation units that include this are built with -ffp-contract=off and correctly rounded fp32 divide / sqrt
// (build.py EXACT), and the double operations used here (convert, multiply, add, sqrt) are IEEE on both sides: everything
// except expf is reproducible on the host bit for bit.
//
// Error bounds.  u = 2^-24 (half an ulp, relative).  Each expression below carries its rounding count c; the bound
// functions at the end turn those counts into c * u * sum|terms|, and are what tests/test_params_cpu.py holds the
// functions to against float64.
#ifndef R3DGS_PARAM_MATH_H
#define R3DGS_PARAM_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

constexpr float kNormalizeEps = 1e-12f;   // F.normalize's eps, rounded to fp32 once (as torch does for fp32 input)

// s = exp(raw).  Device: HIP's expf (<= 1 ulp); host: libm's.  The only function here that is not bit-reproducible.
__host__ __device__ inline float scale_act(float raw) { return expf(raw); }

// dL/draw = dL/ds * s: 1 rounding.   |err| <= 1 u |g s| against the exact product of its fp32 inputs.
__host__ __device__ inline float scale_act_bwd(float g, float s) { return g * s; }

// ||raw||_2 as fp32.  The four squares are exact in double (24-bit x 24-bit significands), the three double sums
// ((x0^2 + x1^2) + x2^2) + x3^2 -- in THIS order -- lose 3 * 2^-53 at most, the double sqrt is correctly rounded: what
// reaches the one fp32 rounding is the exact norm to 2^-52 relative.  1 fp32 rounding: |n - ||raw|| | <= (1 + 2^-27) u n.
// No overflow or underflow for any fp32 input (1e-20 and 1e+15 alike: the squares live in double's range).
__host__ __device__ inline float quat_norm(const float raw[4])
{
    const double x0 = raw[0], x1 = raw[1], x2 = raw[2], x3 = raw[3];
    const double ss = ((x0 * x0 + x1 * x1) + x2 * x2) + x3 * x3;
    return (float)sqrt(ss);
}

// q = raw / max(n, eps): 1 more rounding per component (the divide).  Against the exact quotient: the denominator is off
// by <= u relative (n's rounding; eps's own rounding when the clamp holds), the divide adds u: |err_k| <= 2 u |q_k| (+ second
// order), i.e. less than 2 ulp of q_k.  Returns n.
__host__ __device__ inline float quat_act(const float raw[4], float q[4])
{
    const float n = quat_norm(raw);
    const float den = n > kNormalizeEps ? n : kNormalizeEps;   // max(n, eps)
    q[0] = raw[0] / den;
    q[1] = raw[1] / den;
    q[2] = raw[2] / den;
    q[3] = raw[3] / den;
    return n;
}

// q . g: four products, three sums, sequentially ((q0 g0 + q1 g1) + q2 g2) + q3 g3 -- in THIS order, no fma.
// 4 roundings on the longest path: |err| <= 4 u sum_j |q_j g_j|.
__host__ __device__ inline float quat_dot(const float q[4], const float g[4])
{
    return ((q[0] * g[0] + q[1] * g[1]) + q[2] * g[2]) + q[3] * g[3];
}

// Backward of quat_act.  q, n: what quat_act returned for this raw quaternion (the kernels have both in registers).
//   n >  eps: out_k = (g_k - q_k d) / n,  d = quat_dot(q, g): product (1), difference (1), divide (1) on top of d's 4
//   n <= eps: out_k = g_k / eps: divide (1)
__host__ __device__ inline void quat_act_bwd(const float q[4], float n, const float g[4], float out[4])
{
    if (n > kNormalizeEps) {
        const float d = quat_dot(q, g);
        out[0] = (g[0] - q[0] * d) / n;
        out[1] = (g[1] - q[1] * d) / n;
        out[2] = (g[2] - q[2] * d) / n;
        out[3] = (g[3] - q[3] * d) / n;
    } else {
        out[0] = g[0] / kNormalizeEps;
        out[1] = g[1] / kNormalizeEps;
        out[2] = g[2] / kNormalizeEps;
        out[3] = g[3] / kNormalizeEps;
    }
}

// ---- bounds (host side of the tests; plain double arithmetic) --------------------------------------------------------
constexpr double kUnitRoundoff = 1.0 / 16777216.0;   // u = 2^-24
// A rounding whose result is subnormal (below 2^-126) is not relative any more: it lands on a multiple of 2^-149, half of
// that away at most.  Each rounding counted below adds this absolute term (it only matters for gradients around 1e-38).
constexpr double kSubnormalHalf = 7.006492321624085e-46;   // 2^-150

// scale_act_bwd against the float64 evaluation g * exp(raw): the product's rounding (1) plus s's own distance from
// exp(raw) -- exp_ulps ulp of expf, 2 u each: c = 1 + 2 exp_ulps, on the single term |g s|.
inline double scale_act_bwd_bound(double g, double s, double exp_ulps)
{
    return (1.0 + 2.0 * exp_ulps) * kUnitRoundoff * fabs(g * s) + kSubnormalHalf;
}

// quat_act_bwd, component k, against the float64 evaluation from the same fp32 raw and g.  With S = sum_j |q_j g_j|:
//   d      : inputs q_j off by 2 u each (quat_act) -> 2 u S;  its own arithmetic 4 u S                       => 6 u S
//   q_k d  : q_k off by 2 u, the product's rounding 1 u, on |q_k d| <= |q_k| S; d's error times |q_k|        => 9 u |q_k| S
//   g_k - .: 1 u on |g_k| + |q_k| S
//   / n    : the divide 1 u, n off by 1 u, on the numerator |g_k| + |q_k| S                                   => 2 u (...)
// total: u (3 |g_k| + 12 |q_k| S) / n; one more unit on each count covers the second-order terms: c = 4 and 13.
// Nine roundings could be subnormal (d: 7, product, difference -- all in front of the divide -- and the divide's own).
//   n <= eps: the divide (1) and eps's fp32 rounding (1): c = 2 on |g_k| / eps.
inline double quat_act_bwd_bound(const double q[4], double n, const double g[4], int k)
{
    if (n > (double)kNormalizeEps) {
        const double S = fabs(q[0] * g[0]) + fabs(q[1] * g[1]) + fabs(q[2] * g[2]) + fabs(q[3] * g[3]);
        return kUnitRoundoff * (4.0 * fabs(g[k]) + 13.0 * fabs(q[k]) * S) / n + kSubnormalHalf * (9.0 / n + 1.0);
    }
    return 2.0 * kUnitRoundoff * fabs(g[k]) / 1e-12 + kSubnormalHalf;
}

}  // namespace r3

#endif  // R3DGS_PARAM_MATH_H
