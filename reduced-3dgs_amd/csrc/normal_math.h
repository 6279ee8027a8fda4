// normal_math.h -- per-element arithmetic of the surface-normal unit (normals.hip, include/r3dgs_normals.h): the view-space
// normal of one Gaussian with its backward, and the normal of one pixel of a depth map with its backward.  Shared with the CPU
// test shim tests/hostcheck_normals/hostcheck_normals.hip so the exact source a lane executes is checked without a GPU.
//
// What it restates (restated again, in float64 torch with gradients by autograd, in tests/normals_ref.py):
//   axis      k = argmin of the three scales, the lowest index on a tie (raw log-scales have the same argmin)       normal_axis
//   normal    n_w = column k of R(q) -- the R of quat_to_R / cov3d_from_scale_rot, Sigma = R S^2 R^T -- negated when
//             n_w . (mean - campos) > 0, then taken into the view frame as a row vector times the 3x3 block of the view
//             matrix, the convention of xform4x3                                                                   gaussian_normal_one
//   pixel     z = depth / alpha where alpha >= kNormalAlphaMin, else 0                                             normal_pixel_z
//   ray       r(x, y) = ((2 (x + 0.5) / W - 1) tan_fovx, (2 (y + 0.5) / H - 1) tan_fovy, 1): the pixel centre of ndc2pix
//   depth normal   d_v = p(x, y+1) - p(x, y-1),  d_h = p(x+1, y) - p(x-1, y),  c = d_v x d_h,  n = c / |c|, and n = 0 with a
//             zero gradient when |c|^2 <= kNormalCrossMin (2DGS's depth_to_normal, kept in the view frame)          depth_normal_one
//
// Cancellation-free differences.  With r the centre's ray and (dx, dy) the one-pixel ray step,
//   d_v = (z_b - z_t) r + (z_b + z_t) (0, dy, 0)        d_h = (z_r - z_l) r + (z_r + z_l) (dx, 0, 0)
// instead of the difference of two un-projected points (each ~ z, their difference ~ z / W: three digits lost at 1600 pixels).
//
// Precision.  Everything between the fp32 inputs and the one fp32 rounding of each output runs in double (as mip_math.h): the
// kernels are bandwidth-bound and the arithmetic hides under the loads.  DECISIONS: the argmin on the fp32 scales as given,
// alpha >= kNormalAlphaMin on the fp32 alpha as given, the sign and |c|^2 on the double values.
#ifndef R3DGS_NORMAL_MATH_H
#define R3DGS_NORMAL_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "gauss_math.h"
#include "param_math.h"

namespace r3 {

// Below the smallest alpha a pixel with one blended Gaussian can have (the blend skips alpha < 1/255): the test separates
// "nothing was blended here" from everything else and never divides by noise.
constexpr float kNormalAlphaMin = 1e-3f;
// |c| <= 1e-12, the eps of the normalize in 2DGS's formula: no direction left to normalise.
constexpr float kNormalCrossMin = 1e-24f;

R3_HD int normal_axis(const float* s)
{
    int k = 0;
    if (s[1] < s[0]) k = 1;
    if (s[2] < s[k]) k = 2;
    return k;
}

// Column k of R(q) and its four partial derivatives dcol[4 * i + j] = d col_i / d q_j, q = (r, x, y, z) as given.
R3_HD void rotation_column(const double* q, int k, double* col, double* dcol)
{
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    if (k == 0) {
        col[0] = 1 - 2 * (y * y + z * z), col[1] = 2 * (x * y + r * z), col[2] = 2 * (x * z - r * y);
        const double d[12] = {0, 0, -4 * y, -4 * z, 2 * z, 2 * y, 2 * x, 2 * r, -2 * y, 2 * z, -2 * r, 2 * x};
        for (int e = 0; e < 12; e++) dcol[e] = d[e];
    } else if (k == 1) {
        col[0] = 2 * (x * y - r * z), col[1] = 1 - 2 * (x * x + z * z), col[2] = 2 * (y * z + r * x);
        const double d[12] = {-2 * z, 2 * y, 2 * x, -2 * r, 0, -4 * x, 0, -4 * z, 2 * x, 2 * r, 2 * z, 2 * y};
        for (int e = 0; e < 12; e++) dcol[e] = d[e];
    } else {
        col[0] = 2 * (x * z + r * y), col[1] = 2 * (y * z - r * x), col[2] = 1 - 2 * (x * x + y * y);
        const double d[12] = {2 * y, 2 * z, 2 * r, 2 * x, -2 * x, -2 * r, 2 * z, 2 * y, 0, -4 * x, -4 * y, 0};
        for (int e = 0; e < 12; e++) dcol[e] = d[e];
    }
}

// The quaternion the axis is read from, in double: as given, or -- raw -- divided by max(|q|, eps) like quat_act.
R3_HD double normal_quat(const float* qf, bool raw, double* q)
{
    double den = 1.0;
    if (raw) {
        const double n = sqrt(((double)qf[0] * qf[0] + (double)qf[1] * qf[1]) + (double)qf[2] * qf[2] + (double)qf[3] * qf[3]);
        den = n > (double)kNormalizeEps ? n : (double)kNormalizeEps;
    }
    for (int j = 0; j < 4; j++) q[j] = (double)qf[j] / den;
    return den;
}

// -> the sign applied (+1 / -1); out[3]: the view-space normal.
R3_HD double gaussian_normal_one(const float* view, const float* campos, const float* mean, const float* scale, const float* qf,
                                 bool raw, float* out)
{
    double q[4], col[3], dcol[12];
    normal_quat(qf, raw, q);
    rotation_column(q, normal_axis(scale), col, dcol);
    const double dot = col[0] * ((double)mean[0] - campos[0]) + col[1] * ((double)mean[1] - campos[1]) +
                       col[2] * ((double)mean[2] - campos[2]);
    const double sgn = dot > 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 3; j++)
        out[j] = (float)(sgn * (col[0] * view[j] + col[1] * view[4 + j] + col[2] * view[8 + j]));
    return sgn;
}

// g[3]: dL / d out  ->  dq[4]: dL / d (the quaternion as given).  The axis and the sign are piecewise constant.
R3_HD void gaussian_normal_bwd_one(const float* view, const float* campos, const float* mean, const float* scale, const float* qf,
                                   bool raw, const float* g, float* dq)
{
    double q[4], col[3], dcol[12];
    const double den = normal_quat(qf, raw, q);
    rotation_column(q, normal_axis(scale), col, dcol);
    const double dot = col[0] * ((double)mean[0] - campos[0]) + col[1] * ((double)mean[1] - campos[1]) +
                       col[2] * ((double)mean[2] - campos[2]);
    const double sgn = dot > 0.0 ? -1.0 : 1.0;
    double gq[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 3; i++) {
        const double gc = sgn * ((double)g[0] * view[4 * i] + (double)g[1] * view[4 * i + 1] + (double)g[2] * view[4 * i + 2]);
        for (int j = 0; j < 4; j++) gq[j] += gc * dcol[4 * i + j];
    }
    if (raw) {
        const bool clamped = !(den > (double)kNormalizeEps);
        const double d = clamped ? 0.0 : ((q[0] * gq[0] + q[1] * gq[1]) + q[2] * gq[2]) + q[3] * gq[3];
        for (int j = 0; j < 4; j++) dq[j] = (float)((gq[j] - q[j] * d) / den);
    } else {
        for (int j = 0; j < 4; j++) dq[j] = (float)gq[j];
    }
}

// ---- depth normals ------------------------------------------------------------------------------------------------------------

// The rays of an image: r(x, y) = (x0 + x dx, y0 + y dy, 1).
struct NormalRays {
    double x0, dx, y0, dy;
};
R3_HD NormalRays normal_rays(int W, int H, float tan_fovx, float tan_fovy)
{
    NormalRays r;
    r.dx = 2.0 * (double)tan_fovx / (double)W;
    r.dy = 2.0 * (double)tan_fovy / (double)H;
    r.x0 = (1.0 / (double)W - 1.0) * (double)tan_fovx;   // (2 (0 + 0.5) / W - 1) tan_fovx
    r.y0 = (1.0 / (double)H - 1.0) * (double)tan_fovy;
    return r;
}

R3_HD bool normal_alpha_live(float alpha) { return alpha >= kNormalAlphaMin; }
R3_HD double normal_pixel_z(float depth, float alpha, bool has_alpha)
{
    if (!has_alpha) return (double)depth;
    return normal_alpha_live(alpha) ? (double)depth / (double)alpha : 0.0;
}

struct DepthNormal {
    double n[3], dv[3], dh[3], inv_len;   // inv_len == 0: degenerate, n == 0
};

// zt, zb, zl, zr: z at (x, y-1), (x, y+1), (x-1, y), (x+1, y); (rx, ry): the centre's ray.
R3_HD DepthNormal depth_normal_one(double zt, double zb, double zl, double zr, double rx, double ry, double dx, double dy)
{
    DepthNormal o;
    const double dzv = zb - zt, dzh = zr - zl;
    o.dv[0] = dzv * rx, o.dv[1] = dzv * ry + (zb + zt) * dy, o.dv[2] = dzv;
    o.dh[0] = dzh * rx + (zr + zl) * dx, o.dh[1] = dzh * ry, o.dh[2] = dzh;
    const double c[3] = {o.dv[1] * o.dh[2] - o.dv[2] * o.dh[1], o.dv[2] * o.dh[0] - o.dv[0] * o.dh[2],
                         o.dv[0] * o.dh[1] - o.dv[1] * o.dh[0]};
    const double len2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    o.inv_len = len2 > (double)kNormalCrossMin ? 1.0 / sqrt(len2) : 0.0;
    for (int j = 0; j < 3; j++) o.n[j] = c[j] * o.inv_len;
    return o;
}

// g[3]: dL / d n of this centre  ->  to[4]: its share of dL / dz of the pixel below, above, right of and left of it.
R3_HD void depth_normal_bwd_one(const DepthNormal& o, double rx, double ry, double dx, double dy, const double* g, double* to)
{
    const double ng = o.n[0] * g[0] + o.n[1] * g[1] + o.n[2] * g[2];
    const double gc[3] = {(g[0] - o.n[0] * ng) * o.inv_len, (g[1] - o.n[1] * ng) * o.inv_len, (g[2] - o.n[2] * ng) * o.inv_len};
    // c = d_v x d_h:  dL/d d_v = d_h x gc,  dL/d d_h = gc x d_v
    const double gv[3] = {o.dh[1] * gc[2] - o.dh[2] * gc[1], o.dh[2] * gc[0] - o.dh[0] * gc[2], o.dh[0] * gc[1] - o.dh[1] * gc[0]};
    const double gh[3] = {gc[1] * o.dv[2] - gc[2] * o.dv[1], gc[2] * o.dv[0] - gc[0] * o.dv[2], gc[0] * o.dv[1] - gc[1] * o.dv[0]};
    const double av = gv[0] * rx + gv[1] * ry + gv[2], bv = gv[1] * dy;
    const double ah = gh[0] * rx + gh[1] * ry + gh[2], bh = gh[0] * dx;
    to[0] = av + bv;    // z_b
    to[1] = bv - av;    // z_t
    to[2] = ah + bh;    // z_r
    to[3] = bh - ah;    // z_l
}

// One pixel's term of the consistency loss, w (1 - s N . n), before the division by H W.
R3_HD double normal_loss_term(double w, double s, const float* N, const double* n)
{
    return w * (1.0 - s * ((double)N[0] * n[0] + (double)N[1] * n[1] + (double)N[2] * n[2]));
}

}  // namespace r3

#endif  // R3DGS_NORMAL_MATH_H
