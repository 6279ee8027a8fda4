// camera_math.h -- one Gaussian's share of the camera gradients (include/r3dgs_camera.h r3dgs_camera_backward): the partial
// derivatives of the loss with respect to viewmatrix, projmatrix and campos, taken as three independent inputs, from the
// per-Gaussian screen-space sums the backward wrote (dL_dmean2D, dL_dconic, dL_dcolor).  __host__ __device__ inline, like
// gauss_math.h / aux_math.h: the kernel of camera_bwd.hip runs it per lane, tests/hostcheck_camera/hostcheck_camera.hip
// runs the same source on the CPU against the float64 reference tests/camera_grad_ref.py.
//
// Conventions are r3dgs_backward's (gauss_math.h): flat m[4 * j + i] is entry (row j, column i) of the transposed,
// row-vector matrix the caller passes, so with mt = [m, 1]:  t_i = sum_j V[4 j + i] mt_j,  h_i = sum_j F[4 j + i] mt_j.
//   projmatrix  h -> (h.x, h.y) / (h.w + 1e-7) is all that reads it; dL_dmean2D is in those NDC units.  dL/dF = mt^T dL/dh;
//               column 2 is never read.
//   viewmatrix  through t inside J(t) and through Rw = V[:3,:3]^T in cov2D = (J Rw) Sigma (J Rw)^T + 0.3 I: the chain of
//               cov2d_backward_f64 (conic -> cov2D with its 1 / (det^2 + 1e-7), the clamp masks taken in fp32 as the forward
//               took them, a clamped t.x / t.y a constant times t.z inside J and passing nothing on), continued to V instead
//               of to the mean.  Column 3 is never read; depth order, cull, radius and rect are integer decisions.
//   campos      through the unit view direction of the SH colour: -(I - d d^T) / |m - campos| * (d rgb / d d)^T dL_dcolor,
//               clamped channels left out (sh_backward's dRGB and its dnormvdv).
// T = double or float: the arithmetic of the chain (r3dgs_set_f64_chain).  The sums are double either way.
//
// Layout of the 27 sums: [0, 12) dL/dV rows 0..3 x columns 0..2 (3 j + i); [12, 24) dL/dF rows 0..3 x columns 0, 1, 3
// (3 j + {0, 1, 2}); [24, 27) dL/dcampos.
#pragma once
#include "gauss_math.h"
#include "param_math.h"

namespace r3 {

constexpr int kCamSums = 27;

R3_HD float cam_sqrt(float v) { return sqrtf(v); }
R3_HD double cam_sqrt(double v) { return sqrt(v); }

// the sums -> the three outputs in the inputs' layout, the structurally empty columns zero
R3_HD float camera_view_entry(const double* sums, int k) { return (k & 3) < 3 ? (float)sums[3 * (k >> 2) + (k & 3)] : 0.f; }
R3_HD float camera_proj_entry(const double* sums, int k)
{
    const int i = k & 3;
    return i == 2 ? 0.f : (float)sums[12 + 3 * (k >> 2) + (i == 3 ? 2 : i)];
}

template <class T>
R3_HD void camera_grad_proj(const float* pm, const float* m3, float g2x, float g2y, double* acc)
{
    const T mt[4] = {(T)m3[0], (T)m3[1], (T)m3[2], (T)1};
    T h0 = 0, h1 = 0, h3 = 0;
    for (int j = 0; j < 4; j++) {
        h0 += (T)pm[4 * j] * mt[j];
        h1 += (T)pm[4 * j + 1] * mt[j];
        h3 += (T)pm[4 * j + 3] * mt[j];
    }
    const T mw = (T)1 / (h3 + (T)0.0000001);
    const T dh0 = (T)g2x * mw, dh1 = (T)g2y * mw, dh3 = -(h0 * (T)g2x + h1 * (T)g2y) * mw * mw;
    for (int j = 0; j < 4; j++) {
        acc[12 + 3 * j] += (double)(mt[j] * dh0);
        acc[12 + 3 * j + 1] += (double)(mt[j] * dh1);
        acc[12 + 3 * j + 2] += (double)(mt[j] * dh3);
    }
}

template <class T>
R3_HD void camera_grad_view(const Camera& cam, const float* m3, const float* c6f, float gA, float gB, float gC, double* acc)
{
    const float* vm = cam.view;
    const float mx = m3[0], my = m3[1], mz = m3[2];
    // masks and clamp side from the fp32 evaluation the forward made (ewa_A), as cov2d_backward_f64 takes them
    float tf[3];
    xform4x3(vm, mx, my, mz, tf);
    const float limxf = 1.3f * cam.tan_fovx, limyf = 1.3f * cam.tan_fovy;
    const float txtz = tf[0] / tf[2], tytz = tf[1] / tf[2];
    const bool clx = txtz < -limxf || txtz > limxf, cly = tytz < -limyf || tytz > limyf;
    const T mt[4] = {(T)mx, (T)my, (T)mz, (T)1};
    T t[3];
    for (int r = 0; r < 3; r++) t[r] = (T)vm[r] * mt[0] + (T)vm[4 + r] * mt[1] + (T)vm[8 + r] * mt[2] + (T)vm[12 + r];
    if (clx) t[0] = (txtz < 0.f ? -(T)limxf : (T)limxf) * t[2];
    if (cly) t[1] = (tytz < 0.f ? -(T)limyf : (T)limyf) * t[2];
    const T fx = cam.focal_x, fy = cam.focal_y, itz = (T)1 / t[2], itz2 = itz * itz;
    const T J00 = fx * itz, J02 = -fx * t[0] * itz2, J11 = fy * itz, J12 = -fy * t[1] * itz2;
    T A[6];   // J * Rw, Rw(i,j) = vm[4*j + i]
    for (int j = 0; j < 3; j++) {
        A[j] = J00 * (T)vm[4 * j] + J02 * (T)vm[4 * j + 2];
        A[3 + j] = J11 * (T)vm[4 * j + 1] + J12 * (T)vm[4 * j + 2];
    }
    const T S[9] = {(T)c6f[0], (T)c6f[1], (T)c6f[2], (T)c6f[1], (T)c6f[3], (T)c6f[4], (T)c6f[2], (T)c6f[4], (T)c6f[5]};
    T AS[6];
    for (int i = 0; i < 2; i++)
        for (int k = 0; k < 3; k++) AS[3 * i + k] = A[3 * i] * S[k] + A[3 * i + 1] * S[3 + k] + A[3 * i + 2] * S[6 + k];
    const T a = AS[0] * A[0] + AS[1] * A[1] + AS[2] * A[2] + (T)0.3;
    const T b = AS[0] * A[3] + AS[1] * A[4] + AS[2] * A[5];
    const T c = AS[3] * A[3] + AS[4] * A[4] + AS[5] * A[5] + (T)0.3;
    const T det = a * c - b * b;
    const T k2 = (T)1 / (det * det + (T)0.0000001);
    const T da = k2 * (-c * c * (T)gA + 2 * b * c * (T)gB - b * b * (T)gC);
    const T dc = k2 * (-a * a * (T)gC + 2 * a * b * (T)gB - b * b * (T)gA);
    const T db = k2 * 2 * (b * c * (T)gA - (det + 2 * b * b) * (T)gB + a * b * (T)gC);
    T dA[6];
    for (int j = 0; j < 3; j++) {
        dA[j] = 2 * AS[j] * da + AS[3 + j] * db;
        dA[3 + j] = 2 * AS[3 + j] * dc + AS[j] * db;
    }
    const T dJ00 = (T)vm[0] * dA[0] + (T)vm[4] * dA[1] + (T)vm[8] * dA[2];
    const T dJ02 = (T)vm[2] * dA[0] + (T)vm[6] * dA[1] + (T)vm[10] * dA[2];
    const T dJ11 = (T)vm[1] * dA[3] + (T)vm[5] * dA[4] + (T)vm[9] * dA[5];
    const T dJ12 = (T)vm[2] * dA[3] + (T)vm[6] * dA[4] + (T)vm[10] * dA[5];
    const T itz3 = itz2 * itz;
    T dt[3];
    dt[0] = clx ? (T)0 : -fx * itz2 * dJ02;
    dt[1] = cly ? (T)0 : -fy * itz2 * dJ12;
    dt[2] = -fx * itz2 * dJ00 - fy * itz2 * dJ11 + 2 * fx * t[0] * itz3 * dJ02 + 2 * fy * t[1] * itz3 * dJ12;
    // V[4 j + i] enters t_i with the factor mt_j (every j), and as Rw(i, j) the rows of A (j < 3)
    for (int j = 0; j < 4; j++) {
        T g0 = mt[j] * dt[0], g1 = mt[j] * dt[1], g2 = mt[j] * dt[2];
        if (j < 3) {
            g0 += J00 * dA[j];
            g1 += J11 * dA[3 + j];
            g2 += J02 * dA[j] + J12 * dA[3 + j];
        }
        acc[3 * j] += (double)g0;
        acc[3 * j + 1] += (double)g1;
        acc[3 * j + 2] += (double)g2;
    }
}

// d9: d(colour channel)/d(unit view direction) (sh_dir_derivs), dL_dcolor with the clamped channels left out
template <class T>
R3_HD void camera_grad_campos(const float* campos, const float* m3, const float* d9, uint32_t clamp_bits, const float* dL_dcolor,
                              double* acc)
{
    T ddir[3] = {(T)0, (T)0, (T)0};
    for (int ch = 0; ch < 3; ch++) {
        const T g = ((clamp_bits >> ch) & 1u) ? (T)0 : (T)dL_dcolor[ch];
        ddir[0] += (T)d9[3 * ch] * g;
        ddir[1] += (T)d9[3 * ch + 1] * g;
        ddir[2] += (T)d9[3 * ch + 2] * g;
    }
    // the view direction as sh_backward forms it (fp32 differences of fp32 inputs), auxiliary.h:107-117 dnormvdv
    const T vx = (T)(m3[0] - campos[0]), vy = (T)(m3[1] - campos[1]), vz = (T)(m3[2] - campos[2]);
    const T sum2 = vx * vx + vy * vy + vz * vz;
    const T invsum32 = (T)1 / cam_sqrt(sum2 * sum2 * sum2);
    acc[24] -= (double)(((sum2 - vx * vx) * ddir[0] - vy * vx * ddir[1] - vz * vx * ddir[2]) * invsum32);
    acc[25] -= (double)((-vx * vy * ddir[0] + (sum2 - vy * vy) * ddir[1] - vz * vy * ddir[2]) * invsum32);
    acc[26] -= (double)((-vx * vz * ddir[0] - vy * vz * ddir[1] + (sum2 - vz * vz) * ddir[2]) * invsum32);
}

// Everything a lane does for one VISIBLE Gaussian once its inputs are loaded.
//   sc, q       scales / rotations as the caller holds them (raw: the model's raw parameters, activated here by the functions
//               the raw route uses); ignored when c6_precomp != nullptr
//   g2, gcon    dL_dmean2D (x, y) and dL_dconic (A, B, C: the [P,4] row without its unused third slot)
//   colour      0: no SH colour (colors_precomp), or a Gaussian that was binned into no tile and so has no colour -- nothing
//               for campos;  1: d9_cached holds the forward's sh_dir_derivs;  2: evaluate them from `sh` with the row's degree
template <class T, class ShRow>
R3_HD void camera_grad_gaussian(const Camera& cam, const float* m3, const float* sc, const float* q, const float* c6_precomp,
                                bool raw, const float* g2, const float* gcon, const float* dL_dcolor, uint32_t clamp_bits,
                                int deg, int colour, const float* d9_cached, const ShRow& sh, double* acc)
{
    float c6[6];
    if (c6_precomp) {
        for (int k = 0; k < 6; k++) c6[k] = c6_precomp[k];
    } else if (raw) {
        float s[3], qa[4];
        for (int k = 0; k < 3; k++) s[k] = scale_act(sc[k]);
        quat_act(q, qa);
        cov3d_from_scale_rot(s, cam.scale_modifier, qa, c6);
    } else {
        cov3d_from_scale_rot(sc, cam.scale_modifier, q, c6);
    }
    camera_grad_proj<T>(cam.proj, m3, g2[0], g2[1], acc);
    camera_grad_view<T>(cam, m3, c6, gcon[0], gcon[1], gcon[2], acc);
    if (colour != 0 && deg > 0) {
        float d9[9];
        if (colour == 1) {
            for (int k = 0; k < 9; k++) d9[k] = d9_cached[k];
        } else {
            sh_dir_derivs_at(deg, sh, m3[0], m3[1], m3[2], cam.campos, d9);
        }
        camera_grad_campos<T>(cam.campos, m3, d9, clamp_bits, dL_dcolor, acc);
    }
}

// The camera pass of the replay maps (r3dgs_camera_backward_maps: depth / alpha / median depth, distortion, feature maps):
// one VISIBLE Gaussian's share of the first kCamMapSums sums, from the screen-space sums a _screen map backward wrote.  The
// mean and the conic go the way they go above; no colour, so nothing for campos; and the one path the colour image does not
// have -- the maps read the view depth z = t_2 = sum_j V[4 j + 2] mt_j itself, so dL_dz goes to column 2 of V with the
// factor mt_j.  sc, q: ACTIVATED scales / rotations (ignored when c6_precomp != nullptr).
constexpr int kCamMapSums = 24;

template <class T>
R3_HD void camera_maps_gaussian(const Camera& cam, const float* m3, const float* sc, const float* q, const float* c6_precomp,
                                const float* g2, const float* gcon, float gz, double* acc)
{
    float c6[6];
    if (c6_precomp) {
        for (int k = 0; k < 6; k++) c6[k] = c6_precomp[k];
    } else {
        cov3d_from_scale_rot(sc, cam.scale_modifier, q, c6);
    }
    camera_grad_proj<T>(cam.proj, m3, g2[0], g2[1], acc);
    camera_grad_view<T>(cam, m3, c6, gcon[0], gcon[1], gcon[2], acc);
    const T mt[4] = {(T)m3[0], (T)m3[1], (T)m3[2], (T)1};
    for (int j = 0; j < 4; j++) acc[3 * j + 2] += (double)(mt[j] * (T)gz);
}

}  // namespace r3
