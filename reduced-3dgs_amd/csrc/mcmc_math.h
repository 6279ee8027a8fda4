// mcmc_math.h -- per-Gaussian arithmetic of the 3DGS-MCMC strategy (mcmc.hip, include/r3dgs_mcmc.h): the gated noise term,
// the weights and the draw search of the plan, the ratio clamp and the relocation formula.  Shared with the CPU test shim
// tests/hostcheck_mcmc/hostcheck_mcmc.hip so the exact source a lane executes is checked without a GPU.
//
// What it restates (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", 2024; restated in
// tests/mcmc_ref.py):
//   noise     xyz += scale * gate(o) * (R diag(s)^2 R^T) n,   gate(o) = 1 / (1 + exp(-100 ((1 - o) - 0.995)))      mcmc_noise_delta
//   weights   w = sigmoid(raw opacity), 0 for a dead row (RELOCATE: w <= min_opacity)                                mcmc_weight
//   draw      first index with cdf > u * total                                                                      mcmc_search
//   relocate  o' = 1 - (1 - o)^(1/N),  s' = (o / D) s,  D = sum_i sum_k C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)          mcmc_relocate
// The activations are the library's: stats_sigmoid (stats_math.h), scale_act and quat_act (param_math.h); the rotation rows are
// densify_math.h's.  mcmc.hip is compiled with -ffp-contract=off and correctly rounded fp32 divide and sqrt (build.py EXACT):
// every fp32 operation written here is one rounding, in the order written; expf and logf are the only ones that are not
// bit-reproducible between host and device (<= 1 ulp each).  The relocation's o' and D are double.
#ifndef R3DGS_MCMC_MATH_H
#define R3DGS_MCMC_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "densify_math.h"
#include "param_math.h"
#include "stats_math.h"

namespace r3 {

constexpr int kMcmcMaxRatio = 51;               // R3DGS_MCMC_MAX_RATIO: the binomial table has this many rows
constexpr float kMcmcGateSteep = 100.f;         // the gate's slope ...
constexpr float kMcmcGateCentre = 0.995f;       // ... and centre: 1/2 at o = 0.005
constexpr float kMcmcMaxOpacity = 0.99999988079071044921875f;   // 1 - 2^-23: the logit stays finite

// C(n, k) for n, k < 51, exact: the largest, C(50, 25) = 1.26e14, is below 2^53.
struct McmcBinom {
    double c[kMcmcMaxRatio][kMcmcMaxRatio];
};
constexpr McmcBinom make_mcmc_binom()
{
    McmcBinom t{};
    for (int n = 0; n < kMcmcMaxRatio; n++) {
        t.c[n][0] = 1.0;
        for (int k = 1; k <= n; k++) t.c[n][k] = t.c[n - 1][k - 1] + (k <= n - 1 ? t.c[n - 1][k] : 0.0);
    }
    return t;
}

// The gate of the noise term.  Roundings: the two subtractions, the multiply, expf (<= 1 ulp), the add, the divide.  An
// opaque Gaussian's exponent overflows to inf and the gate is 0.
__host__ __device__ inline float mcmc_gate(float o)
{
    return 1.f / (1.f + expf(-kMcmcGateSteep * ((1.f - o) - kMcmcGateCentre)));
}

// scale * gate * (R diag(s)^2 R^T) n for one Gaussian, never forming the covariance: v = R^T n, v_j *= s_j^2, d = R v.
// Sums in THIS order, no fma: (a + b) + c.
__host__ __device__ inline void mcmc_noise_delta(const float raw_q[4], const float raw_scale[3], float raw_opacity,
                                                 const float n[3], float scale, float out[3])
{
    float q[4], R[3][3];
    quat_act(raw_q, q);
    rotation_row(q, 0, R[0]);
    rotation_row(q, 1, R[1]);
    rotation_row(q, 2, R[2]);
    const float g = scale * mcmc_gate(stats_sigmoid(raw_opacity));
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float s = scale_act(raw_scale[j]);
        v[j] = ((R[0][j] * n[0] + R[1][j] * n[1]) + R[2][j] * n[2]) * (s * s);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = g * ((R[k][0] * v[0] + R[k][1] * v[1]) + R[k][2] * v[2]);
}

// x + d, except that a zero displacement leaves the bits of x alone (-0 + 0 would turn into +0).
__host__ __device__ inline float mcmc_displace(float x, float d) { return d == 0.f ? x : x + d; }

// The weight of one row of the plan, and whether the row is dead (relocate != 0 only).
__host__ __device__ inline float mcmc_weight(float raw_opacity, float min_opacity, int relocate, bool& dead)
{
    const float w = stats_sigmoid(raw_opacity);
    dead = relocate && w <= min_opacity;
    return dead ? 0.f : w;
}

// What a draw looks for: u in [0,1) times the total weight, in double (u < 1 has 24 bits: the product is below the total).
__host__ __device__ inline double mcmc_target(float u, double total) { return (double)u * total; }

// First m in [0, n) with cdf[m] > t; n - 1 if there is none.  The result m satisfies cdf[m] > t >= cdf[m - 1] whenever an
// entry above t exists, whether or not cdf is monotone to the last bit.  n >= 1.
__host__ __device__ inline int mcmc_search(const double* cdf, int n, double t)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cdf[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__host__ __device__ inline int mcmc_ratio_clamp(int r) { return r > kMcmcMaxRatio ? kMcmcMaxRatio : r; }

// o' and D of a source of activated opacity o drawn N - 1 times (2 <= N <= 51), in double.  o' through log1p / expm1: no
// cancellation for small o.  The double sum as written, i outer: at most 1326 terms, alternating, up to about (1 + o')^50.
__host__ __device__ inline void mcmc_relocate_f64(double o, int N, const McmcBinom& b, double& o_new, double& D)
{
    o_new = -expm1(log1p(-o) / (double)N);
    double sum = 0.0;
    for (int i = 1; i <= N; i++) {
        double p = 1.0;
        for (int k = 0; k < i; k++) {
            p *= o_new;   // o'^(k+1)
            const double term = b.c[i - 1][k] * p / sqrt((double)(k + 1));
            sum += (k & 1) ? -term : term;
        }
    }
    D = sum;
}

// The new raw opacity and raw scaling of a drawn source.  fp32 roundings: stats_sigmoid's; o' and o / D rounded from double
// once each; the clamp; 1 - o', the divide, logf (opacity); expf, the multiply, logf (each scale).
__host__ __device__ inline void mcmc_relocate(float raw_opacity, const float raw_scale[3], int N, float min_opacity,
                                              const McmcBinom& b, float& new_opacity, float new_scale[3])
{
    const float o = stats_sigmoid(raw_opacity);
    double o_new, D;
    mcmc_relocate_f64((double)o, N, b, o_new, D);
    const float coeff = (float)((double)o / D);
    float of = (float)o_new;
    of = fminf(fmaxf(of, min_opacity), kMcmcMaxOpacity);
    new_opacity = logf(of / (1.f - of));
#pragma unroll
    for (int k = 0; k < 3; k++) new_scale[k] = logf(coeff * scale_act(raw_scale[k]));
}

}  // namespace r3

#endif  // R3DGS_MCMC_MATH_H
