// mip_math.h -- per-Gaussian arithmetic of the anti-aliasing unit (mip.hip, include/r3dgs_mip.h): the per-view 2D opacity
// compensation and its backward, the validity test of the 3D filter, and the 3D smoothing filter's map of the raw parameters
// with its backward.  Shared with the CPU test shim tests/hostcheck_mip/hostcheck_mip.hip so the exact source a lane executes
// is checked without a GPU.
//
// What it restates (restated again, in float64 torch with gradients by autograd, in tests/mip_ref.py):
//   compensation   rho = sqrt(max(0.000025, det(C) / det(C + 0.3 I))),  p = sigmoid(o) rho,  raw_eff = logit(p)     mip_opacity_one
//                  C = (a, b, c): the 2D covariance the forward dilates -- the expressions of gauss_math.h's ewa_A (with the
//                  1.3 tan(fov) clamp), cov2d WITHOUT its two "+ 0.3f" and cov3d_from_scale_rot (with scale_modifier).  These
//                  are the `antialiasing` semantics of the official rasterizer (gsplat's with eps2d = 0.3), NOT Mip-Splatting's
//                  0.1 kernel.
//   3D filter      a camera is valid for a Gaussian if z > 0.2 and the projection lies within 15 % of the image      mip_filter_valid
//   filtered       ls_eff = 0.5 log(exp(2 ls) + f^2),  coef = sqrt(prod s^2 / prod (s^2 + f^2)),
//                  raw_eff = logit(sigmoid(o) coef);  f == 0 copies the inputs bit for bit                           mip_filtered_one
//
// Precision.  a c - b^2 cancels for a needle (scale ratio 1e3: 6 digits), so -- like cov2d_backward_f64 / cov3d_backward_f64 of
// gauss_math.h -- everything between the fp32 inputs and the one fp32 rounding of each output runs in double: the projection, both
// determinants, the logit and the whole backward chain.  DECISIONS are the forward's own: the near-plane cull (z <= 0.2) and the
// clamp masks are taken on the fp32 values preprocess_one / ewa_A form, and the focal lengths and clamp limits are the fp32
// numbers the forward uses.  The kernels are HBM-bound and P-sized; the double arithmetic hides under the loads.
//
// Cancelled forms.  With s = sigmoid(o), p = s rho:  d logit(p) / d o = s (1 - s) / (p (1 - p)) = (1 - s) / (1 - p), and
// d logit(p) / d rho = 1 / (rho (1 - p)): nothing divides by p (1 - p).  1 - s is formed as e / (1 + e), e = exp(-o), without a
// subtraction; 1 - p is floored at 2^-24, the distance from 1 to the largest fp32 number below it.
#ifndef R3DGS_MIP_MATH_H
#define R3DGS_MIP_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "gauss_math.h"
#include "param_math.h"

namespace r3 {

constexpr double kMipDilation = 0.3;          // the forward's low-pass (cov2d: "+ 0.3f" on the diagonal)
constexpr double kMipRatioFloor = 0.000025;   // floor of det(C) / det(C + 0.3 I): rho >= 0.005
constexpr double kMipOneMinusPFloor = 5.9604644775390625e-08;   // 2^-24
constexpr float kMipNear = 0.2f;              // the near plane of every forward (preprocess_one)
constexpr float kMipFilterVar = 0.2f;         // the 3D filter's variance in pixels^2 (Mip-Splatting)
constexpr float kMipFilterMargin = 0.15f;     // a camera sees a Gaussian up to 15 % outside its image

// One view as the compensation reads it.  focal_* as load_camera forms them: W / (2.0f * tan_fovx) in fp32.
struct MipView {
    const float* view;   // [16] world -> view, where the caller keeps it (the kernels: LDS)
    float tan_fovx, tan_fovy, focal_x, focal_y, scale_modifier;
};

__host__ __device__ inline MipView mip_make_view(const float* view, float tan_fovx, float tan_fovy, int W, int H,
                                                 float scale_modifier)
{
    MipView v;
    v.view = view;
    v.tan_fovx = tan_fovx;
    v.tan_fovy = tan_fovy;
    v.focal_x = W / (2.0f * tan_fovx);
    v.focal_y = H / (2.0f * tan_fovy);
    v.scale_modifier = scale_modifier;
    return v;
}

// logit(p) for p = s * m, s = sigmoid(o), m in [0, 1], and the two cancelled factors.  omp: 1 - p, floored.
struct MipLogit {
    double raw;        // log(p) - log(1 - p)
    double d_o;        // d raw / d o = (1 - s) / (1 - p)
    double inv_omp;    // 1 / (1 - p): d raw / d m = inv_omp / m
};
__host__ __device__ inline MipLogit mip_logit(float o, double m)
{
    const double e = exp(-(double)o);     // may be inf (o = -1000): s = 0, 1 - s = 1
    const double s = 1.0 / (1.0 + e);
    const double oms = e > 1.79e308 ? 1.0 : e / (1.0 + e);
    const double p = s * m;
    double omp = 1.0 - p;
    if (!(omp > kMipOneMinusPFloor)) omp = kMipOneMinusPFloor;
    MipLogit r;
    r.raw = log(p) - log(omp);
    r.d_o = oms / omp;
    r.inv_omp = 1.0 / omp;
    return r;
}

// The undilated 2D covariance of one Gaussian in double, with everything its backward needs.
struct MipCov {
    double A[6];      // J * Rw (2x3), the clamp applied
    double AS[6];     // A Sigma
    double S6[6];     // Sigma (00,01,02,11,12,22), the modifier applied
    double t[3];      // view-space mean, the clamp applied to t[0], t[1]
    double a, b, c;   // C = A Sigma A^T
    bool clx, cly;    // the forward's clamp masks (fp32 decisions)
};

// Sigma = R diag(mod s)^2 R^T in double from the fp32 (activated) scale and quaternion: cov3d_from_scale_rot's expression.
__host__ __device__ inline void mip_cov3d(const float* scale, float mod, const float* qf, double* S6)
{
    const double r = qf[0], x = qf[1], y = qf[2], z = qf[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)};
    const double s[3] = {(double)mod * scale[0], (double)mod * scale[1], (double)mod * scale[2]};
    // M[3*k + j] = s_k R(j,k), written out: indexed at run time the arrays would land in scratch
    const double M[9] = {s[0] * R[0], s[0] * R[3], s[0] * R[6], s[1] * R[1], s[1] * R[4], s[1] * R[7],
                         s[2] * R[2], s[2] * R[5], s[2] * R[8]};
#define R3_MIP_SIG(p, q) (M[p] * M[q] + M[3 + p] * M[3 + q] + M[6 + p] * M[6 + q])
    S6[0] = R3_MIP_SIG(0, 0);
    S6[1] = R3_MIP_SIG(0, 1);
    S6[2] = R3_MIP_SIG(0, 2);
    S6[3] = R3_MIP_SIG(1, 1);
    S6[4] = R3_MIP_SIG(1, 2);
    S6[5] = R3_MIP_SIG(2, 2);
#undef R3_MIP_SIG
}

// ewa_A and cov2d (without the dilation) in double; the clamp masks and sides from the fp32 evaluation ewa_A makes.
// tf: the fp32 view-space mean (xform4x3), which the caller has already formed for the cull.
__host__ __device__ inline void mip_cov2d(const MipView& v, const float* m, const float* tf, MipCov& o)
{
    const float* vm = v.view;
    const float limxf = 1.3f * v.tan_fovx, limyf = 1.3f * v.tan_fovy;
    const float txtz = tf[0] / tf[2], tytz = tf[1] / tf[2];
    o.clx = txtz < -limxf || txtz > limxf;
    o.cly = tytz < -limyf || tytz > limyf;
    for (int r = 0; r < 3; r++)
        o.t[r] = (double)vm[r] * m[0] + (double)vm[4 + r] * m[1] + (double)vm[8 + r] * m[2] + (double)vm[12 + r];
    if (o.clx) o.t[0] = (txtz < 0.f ? -(double)limxf : (double)limxf) * o.t[2];
    if (o.cly) o.t[1] = (tytz < 0.f ? -(double)limyf : (double)limyf) * o.t[2];
    const double fx = v.focal_x, fy = v.focal_y, itz = 1.0 / o.t[2], itz2 = itz * itz;
    const double J00 = fx * itz, J02 = -fx * o.t[0] * itz2, J11 = fy * itz, J12 = -fy * o.t[1] * itz2;
    for (int j = 0; j < 3; j++) {   // Rw(i,j) = vm[4*j + i]
        o.A[j] = J00 * vm[4 * j] + J02 * vm[4 * j + 2];
        o.A[3 + j] = J11 * vm[4 * j + 1] + J12 * vm[4 * j + 2];
    }
    const double* c6 = o.S6;
    // AS = A Sigma, written out (a loop over a local copy of Sigma as a 3x3 array is indexed at run time and lands in scratch)
    o.AS[0] = o.A[0] * c6[0] + o.A[1] * c6[1] + o.A[2] * c6[2];
    o.AS[1] = o.A[0] * c6[1] + o.A[1] * c6[3] + o.A[2] * c6[4];
    o.AS[2] = o.A[0] * c6[2] + o.A[1] * c6[4] + o.A[2] * c6[5];
    o.AS[3] = o.A[3] * c6[0] + o.A[4] * c6[1] + o.A[5] * c6[2];
    o.AS[4] = o.A[3] * c6[1] + o.A[4] * c6[3] + o.A[5] * c6[4];
    o.AS[5] = o.A[3] * c6[2] + o.A[4] * c6[4] + o.A[5] * c6[5];
    o.a = o.AS[0] * o.A[0] + o.AS[1] * o.A[1] + o.AS[2] * o.A[2];
    o.b = o.AS[0] * o.A[3] + o.AS[1] * o.A[4] + o.AS[2] * o.A[5];
    o.c = o.AS[3] * o.A[3] + o.AS[4] * o.A[4] + o.AS[5] * o.A[5];
}

// det(C) / det(C + 0.3 I), both determinants in double.  det(C + 0.3 I) >= 0.09 for a positive semi-definite C.
__host__ __device__ inline double mip_det_ratio(double a, double b, double c, double* det, double* det_d)
{
    *det = a * c - b * b;
    *det_d = (a + kMipDilation) * (c + kMipDilation) - b * b;
    return *det / *det_d;
}

// The forward of one Gaussian.  scale / q: ACTIVATED; cov6: the precomputed covariance or nullptr.
// -> raw_eff; *rho_out (may be nullptr).  A Gaussian every forward culls (view z <= 0.2) keeps its raw opacity, rho = 1.
__host__ __device__ inline float mip_opacity_one(const MipView& v, const float* m, const float* scale, const float* q,
                                                 const float* cov6, float o, float* rho_out)
{
    float tf[3];
    xform4x3(v.view, m[0], m[1], m[2], tf);
    if (tf[2] <= kMipNear) {
        if (rho_out) *rho_out = 1.f;
        return o;
    }
    MipCov C;
    if (cov6) {
        for (int k = 0; k < 6; k++) C.S6[k] = cov6[k];
    } else {
        mip_cov3d(scale, v.scale_modifier, q, C.S6);
    }
    mip_cov2d(v, m, tf, C);
    double det, det_d;
    const double ratio = mip_det_ratio(C.a, C.b, C.c, &det, &det_d);
    const double rho = sqrt(ratio > kMipRatioFloor ? ratio : kMipRatioFloor);
    if (rho_out) *rho_out = (float)rho;
    return (float)mip_logit(o, rho).raw;
}

// The backward of one Gaussian from g = dL/draw_eff.  Outputs: d_o, dmean[3], and either dscale[3] (w.r.t. the ACTIVATED
// scale as it was handed in, the modifier's factor included) + dq[4] (w.r.t. the quaternion as handed in: no normalisation
// Jacobian, as cov3d_backward), or -- cov6 != nullptr -- dcov6[6] (off-diagonals: the sum of both symmetric entries, the
// convention of dL_dcov3D).  Everything not produced is zero.
__host__ __device__ inline void mip_opacity_bwd_one(const MipView& v, const float* m, const float* scale, const float* q,
                                                    const float* cov6, float o, float g, float* d_o, float* dmean, float* dscale,
                                                    float* dq, float* dcov6)
{
    for (int k = 0; k < 3; k++) dmean[k] = dscale[k] = 0.f;
    for (int k = 0; k < 4; k++) dq[k] = 0.f;
    for (int k = 0; k < 6; k++) dcov6[k] = 0.f;
    float tf[3];
    xform4x3(v.view, m[0], m[1], m[2], tf);
    if (tf[2] <= kMipNear) {
        *d_o = g;
        return;
    }
    MipCov C;
    if (cov6) {
        for (int k = 0; k < 6; k++) C.S6[k] = cov6[k];
    } else {
        mip_cov3d(scale, v.scale_modifier, q, C.S6);
    }
    mip_cov2d(v, m, tf, C);
    double det, det_d;
    const double ratio = mip_det_ratio(C.a, C.b, C.c, &det, &det_d);
    const bool floored = !(ratio > kMipRatioFloor);
    const double rho = sqrt(floored ? kMipRatioFloor : ratio);
    const MipLogit L = mip_logit(o, rho);
    *d_o = (float)((double)g * L.d_o);
    if (floored) return;   // below the floor rho is a constant
    // d raw / d ratio = 1 / (rho (1 - p)) * 1 / (2 rho)
    const double gr = (double)g * L.inv_omp / (2.0 * ratio);
    // d ratio / d(a, b, c);  b: the off-diagonal entry, which C holds twice
    const double id2 = 1.0 / (det_d * det_d);
    const double da = gr * (C.c * det_d - det * (C.c + kMipDilation)) * id2;
    const double dc = gr * (C.a * det_d - det * (C.a + kMipDilation)) * id2;
    const double db = gr * (-2.0 * C.b * (det_d - det)) * id2;
    const double* A = C.A;
    double G6[6];   // dL/dSigma in the 6-vector convention
    G6[0] = A[0] * A[0] * da + A[0] * A[3] * db + A[3] * A[3] * dc;
    G6[3] = A[1] * A[1] * da + A[1] * A[4] * db + A[4] * A[4] * dc;
    G6[5] = A[2] * A[2] * da + A[2] * A[5] * db + A[5] * A[5] * dc;
    G6[1] = 2 * A[0] * A[1] * da + (A[0] * A[4] + A[1] * A[3]) * db + 2 * A[3] * A[4] * dc;
    G6[2] = 2 * A[0] * A[2] * da + (A[0] * A[5] + A[2] * A[3]) * db + 2 * A[3] * A[5] * dc;
    G6[4] = 2 * A[2] * A[1] * da + (A[1] * A[5] + A[2] * A[4]) * db + 2 * A[4] * A[5] * dc;
    // C = A Sigma A^T -> dL/dA, then J, t and the mean (the chain of cov2d_backward_f64 from here on)
    double dA[6];
    for (int j = 0; j < 3; j++) {
        dA[j] = 2 * C.AS[j] * da + C.AS[3 + j] * db;
        dA[3 + j] = 2 * C.AS[3 + j] * dc + C.AS[j] * db;
    }
    const float* vm = v.view;
    const double dJ00 = vm[0] * dA[0] + vm[4] * dA[1] + vm[8] * dA[2];
    const double dJ02 = vm[2] * dA[0] + vm[6] * dA[1] + vm[10] * dA[2];
    const double dJ11 = vm[1] * dA[3] + vm[5] * dA[4] + vm[9] * dA[5];
    const double dJ12 = vm[2] * dA[3] + vm[6] * dA[4] + vm[10] * dA[5];
    const double fx = v.focal_x, fy = v.focal_y, itz = 1.0 / C.t[2], itz2 = itz * itz, itz3 = itz2 * itz;
    const double dtx = C.clx ? 0.0 : -fx * itz2 * dJ02;
    const double dty = C.cly ? 0.0 : -fy * itz2 * dJ12;
    // a clamped t[0] = +-lim * t[2] moves with t[2]: J02 = -fx t[0] / t[2]^2 = -+fx lim / t[2]
    double dtz = -fx * itz2 * dJ00 - fy * itz2 * dJ11;
    dtz += C.clx ? fx * C.t[0] * itz3 * dJ02 : 2 * fx * C.t[0] * itz3 * dJ02;
    dtz += C.cly ? fy * C.t[1] * itz3 * dJ12 : 2 * fy * C.t[1] * itz3 * dJ12;
    dmean[0] = (float)(vm[0] * dtx + vm[1] * dty + vm[2] * dtz);
    dmean[1] = (float)(vm[4] * dtx + vm[5] * dty + vm[6] * dtz);
    dmean[2] = (float)(vm[8] * dtx + vm[9] * dty + vm[10] * dtz);
    if (cov6) {
        for (int k = 0; k < 6; k++) dcov6[k] = (float)G6[k];
        return;
    }
    float ds[3];
    cov3d_backward_f64(scale, v.scale_modifier, q, G6, ds, dq);   // ds: w.r.t. mod * scale
    for (int k = 0; k < 3; k++) dscale[k] = (float)((double)v.scale_modifier * ds[k]);
}

// ---- 3D filter -------------------------------------------------------------------------------------------------------------

constexpr int kMipCamFloats = 20;   // a row of the camera table: world_view_transform (16), focal_x, focal_y, W, H

// Camera `cam` against the Gaussian at m.  -> view z if the camera is valid for it (z > 0.2 and both projections within
// [-0.15 S, 1.15 S]), else 0.  In double, and without a divide: for z > 0,  lo <= x / z * f + S / 2 <= hi  <=>
// (lo - S / 2) z <= x f <= (hi - S / 2) z.
__host__ __device__ inline float mip_filter_valid(const float* cam, const float* m)
{
    double t[3];
    for (int r = 0; r < 3; r++)
        t[r] = (double)cam[r] * m[0] + (double)cam[4 + r] * m[1] + (double)cam[8 + r] * m[2] + (double)cam[12 + r];
    if (!(t[2] > (double)kMipNear)) return 0.f;
    const double fx = cam[16], fy = cam[17], W = cam[18], H = cam[19];
    const double lo = -(double)kMipFilterMargin - 0.5, hi = 1.0 + (double)kMipFilterMargin - 0.5;
    const double px = t[0] * fx, py = t[1] * fy;
    const bool in = px >= lo * W * t[2] && px <= hi * W * t[2] && py >= lo * H * t[2] && py <= hi * H * t[2];
    return in ? (float)t[2] : 0.f;
}

// filter = d / max focal * sqrt(0.2): the divide, then the multiply by sqrt(0.2) rounded to fp32 once.
__host__ __device__ inline float mip_filter_value(float d, float focal_max)
{
    return (d / focal_max) * 0.4472135954999579f;
}

// ---- the 3D filter applied to the raw parameters -------------------------------------------------------------------------

// ls[3], o, f -> ls_eff[3], raw_eff.  f == 0: the inputs, bit for bit.
__host__ __device__ inline void mip_filtered_one(const float* ls, float o, float f, float* ls_eff, float* raw_eff)
{
    if (f == 0.f) {
        for (int k = 0; k < 3; k++) ls_eff[k] = ls[k];
        *raw_eff = o;
        return;
    }
    const double f2 = (double)f * (double)f;
    double prod = 1.0;
    for (int k = 0; k < 3; k++) {
        const double s2 = exp(2.0 * (double)ls[k]);
        ls_eff[k] = (float)(0.5 * log(s2 + f2));
        prod *= s2 / (s2 + f2);
    }
    *raw_eff = (float)mip_logit(o, sqrt(prod)).raw;
}

// g_ls[3] = dL/dls_eff, g_o = dL/draw_eff -> d_ls[3], d_o.  f carries no gradient.
//   d ls_eff_k / d ls_k = s_k^2 / (s_k^2 + f^2) =: w_k       d log coef / d ls_k = 1 - w_k = f^2 / (s_k^2 + f^2)
//   d raw_eff / d ls_k = (1 - w_k) / (1 - p)                  d raw_eff / d o = (1 - sigmoid(o)) / (1 - p)
__host__ __device__ inline void mip_filtered_bwd_one(const float* ls, float o, float f, const float* g_ls, float g_o, float* d_ls,
                                                     float* d_o)
{
    if (f == 0.f) {
        for (int k = 0; k < 3; k++) d_ls[k] = g_ls[k];
        *d_o = g_o;
        return;
    }
    const double f2 = (double)f * (double)f;
    double prod = 1.0, w[3], omw[3];
    for (int k = 0; k < 3; k++) {
        const double s2 = exp(2.0 * (double)ls[k]);
        w[k] = s2 / (s2 + f2);
        omw[k] = f2 / (s2 + f2);
        prod *= w[k];
    }
    const MipLogit L = mip_logit(o, sqrt(prod));
    for (int k = 0; k < 3; k++) d_ls[k] = (float)((double)g_ls[k] * w[k] + (double)g_o * omw[k] * L.inv_omp);
    *d_o = (float)((double)g_o * L.d_o);
}

}  // namespace r3

#endif  // R3DGS_MIP_MATH_H
