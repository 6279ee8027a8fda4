// exposure_math.h -- per-pixel arithmetic of the exposure + mask stage in front of the fused loss (loss.hip's exposure kernels),
// shared with the CPU test shim tests/hostcheck_exposure/hostcheck_exposure.hip so the source a lane executes is checked
// without a GPU.
//
// The official per-image exposure (3DGS train.py, Oct 2024): E is a 3 x 4 row-major matrix,
//   x'_c  = sum_k E[k][c] x_k + E[c][3]          (the pixel as a row vector times E[:, :3], plus the last column)
//   x''_c = m x'_c                               (m: the pixel's mask weight)
// and its adjoint for an upstream gradient g_c = dL/dx''_c:
//   dx_k      = m sum_c E[k][c] g_c
//   dE[k][c] += (m g_c) x_k                      (k < 3)
//   dE[c][3] += (m g_c)
//
// The evaluation order is fixed here and does not depend on a translation unit's contraction flags: the diagonal term first (a
// plain product), then the other two in rising index (each an explicit fmaf), then the offset (a plain sum), the mask last; the
// function that holds the plain steps switches contraction off for its own body, so no flag can fuse them.  A coefficient that is
// exactly zero contributes NOTHING (its term is skipped, not multiplied): with E = eye(3,4) and m = 1 the map returns x_c
// and the adjoint returns g_k bit for bit, the sign of a zero included, whatever the other channels hold.
#ifndef R3DGS_EXPOSURE_MATH_H
#define R3DGS_EXPOSURE_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

constexpr int kExposureFloats = 12;   // one image's E, [3][4] row-major

// acc + e * v, or acc where e is exactly zero
__host__ __device__ inline float exposure_madd(float e, float v, float acc)
{
    return e == 0.f ? acc : fmaf(e, v, acc);
}

// the two indices of {0, 1, 2} other than i, rising
__host__ __device__ inline int exposure_other_a(int i) { return i == 0 ? 1 : 0; }
__host__ __device__ inline int exposure_other_b(int i) { return i == 2 ? 1 : 2; }

// The one product-sum of the map and of its adjoint: m (ed vd + ea va + eb vb + off), in that order; (ed, vd) is the diagonal
// pair, (ea, va) and (eb, vb) the other two in rising index.
__host__ __device__ inline float exposure_sum(float ed, float ea, float eb, float off, float vd, float va, float vb, float m)
{
#pragma clang fp contract(off)   // the plain product and the plain sum below stay a product and a sum under any unit's flags
    float t = ed * vd;
    t = exposure_madd(ea, va, t);
    t = exposure_madd(eb, vb, t);
    return m * (off == 0.f ? t : t + off);
}

// x''_c = m (sum_k E[k][c] x_k + E[c][3])
__host__ __device__ inline float exposed(const float* E, float x0, float x1, float x2, float m, int c)
{
    const int a = exposure_other_a(c), b = exposure_other_b(c);
    const float xd = c == 0 ? x0 : (c == 1 ? x1 : x2), xa = a == 0 ? x0 : x1, xb = b == 1 ? x1 : x2;
    return exposure_sum(E[4 * c + c], E[4 * a + c], E[4 * b + c], E[4 * c + 3], xd, xa, xb, m);
}

// dx_k = m sum_c E[k][c] g_c
__host__ __device__ inline float exposed_adjoint(const float* E, float g0, float g1, float g2, float m, int k)
{
    const int a = exposure_other_a(k), b = exposure_other_b(k);
    const float gd = k == 0 ? g0 : (k == 1 ? g1 : g2), ga = a == 0 ? g0 : g1, gb = b == 1 ? g1 : g2;
    return exposure_sum(E[4 * k + k], E[4 * k + a], E[4 * k + b], 0.f, gd, ga, gb, m);
}

// the twelve terms of one pixel added to dE[3][4] (double): dE[k][c] += (m g_c) x_k, dE[c][3] += m g_c
__host__ __device__ inline void exposure_grad_accumulate(double (&dE)[kExposureFloats], float x0, float x1, float x2, float g0,
                                                         float g1, float g2, float m)
{
    const double x[3] = {(double)x0, (double)x1, (double)x2};
    const double mg[3] = {(double)m * (double)g0, (double)m * (double)g1, (double)m * (double)g2};
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int k = 0; k < 3; k++) dE[4 * k + c] = fma(mg[c], x[k], dE[4 * k + c]);
        dE[4 * c + 3] += mg[c];
    }
}

}  // namespace r3

#endif  // R3DGS_EXPOSURE_MATH_H
