// hostcheck_mip.hip -- TEST SHIM: runs the product's per-Gaussian anti-aliasing arithmetic (reduced-3dgs_amd/csrc/mip_math.h, the
// __host__ __device__ functions csrc/mip.hip executes per lane) on the CPU, so tests/test_mip_cpu.py can compare it with the
// float64 restatement WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
// Built twice: as a shared library the test loads with ctypes, and -- with -DHOSTCHECK_MIP_MAIN -- as a stand-alone program
// that sweeps the same functions over edge inputs, which the test also compiles with -fsanitize=address,undefined on the host
// side and runs on its own (nothing that carries a sanitizer is loaded into Python).
#include "../../reduced-3dgs_amd/csrc/mip_math.h"

#include <cstdio>
#include <vector>

extern "C" {

// opacity_kernel's per-lane body.  raw != 0: scales / rotations are the model's raw tensors.  cov6 may be NULL.
void hc_mip_opacity(int n, const float* means, const float* scales, const float* rotations, const float* cov6, const float* opac,
                    int raw, const float* view, float tan_fovx, float tan_fovy, int W, int H, float mod, float* raw_eff, float* rho)
{
    const r3::MipView v = r3::mip_make_view(view, tan_fovx, tan_fovy, W, H, mod);
    for (int i = 0; i < n; i++) {
        float s[3] = {1.f, 1.f, 1.f}, q[4] = {1.f, 0.f, 0.f, 0.f};
        if (!cov6) {
            for (int k = 0; k < 3; k++) s[k] = raw ? r3::scale_act(scales[3 * i + k]) : scales[3 * i + k];
            if (raw)
                r3::quat_act(rotations + 4 * i, q);
            else
                for (int k = 0; k < 4; k++) q[k] = rotations[4 * i + k];
        }
        raw_eff[i] = r3::mip_opacity_one(v, means + 3 * i, s, q, cov6 ? cov6 + 6 * i : nullptr, opac[i], rho + i);
    }
}

// opacity_bwd_kernel's per-lane body
void hc_mip_opacity_bwd(int n, const float* means, const float* scales, const float* rotations, const float* cov6,
                        const float* opac, int raw, const float* view, float tan_fovx, float tan_fovy, int W, int H, float mod,
                        const float* g, float* d_o, float* d_means, float* d_scales, float* d_rot, float* d_cov)
{
    const r3::MipView v = r3::mip_make_view(view, tan_fovx, tan_fovy, W, H, mod);
    for (int i = 0; i < n; i++) {
        float s[3] = {1.f, 1.f, 1.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, nrm = 1.f;
        if (!cov6) {
            for (int k = 0; k < 3; k++) s[k] = raw ? r3::scale_act(scales[3 * i + k]) : scales[3 * i + k];
            if (raw)
                nrm = r3::quat_act(rotations + 4 * i, q);
            else
                for (int k = 0; k < 4; k++) q[k] = rotations[4 * i + k];
        }
        float ds[3], dq[4];
        r3::mip_opacity_bwd_one(v, means + 3 * i, s, q, cov6 ? cov6 + 6 * i : nullptr, opac[i], g[i], d_o + i, d_means + 3 * i, ds,
                                dq, d_cov + 6 * i);
        if (raw) {
            float dq_raw[4];
            r3::quat_act_bwd(q, nrm, dq, dq_raw);
            for (int k = 0; k < 4; k++) dq[k] = dq_raw[k];
            for (int k = 0; k < 3; k++) ds[k] = r3::scale_act_bwd(ds[k], s[k]);
        }
        for (int k = 0; k < 3; k++) d_scales[3 * i + k] = ds[k];
        for (int k = 0; k < 4; k++) d_rot[4 * i + k] = dq[k];
    }
}

// the two filter3d kernels, sequentially
void hc_mip_filter3d(int n, int V, const float* means, const float* cams, float* filter)
{
    float focal_max = 0.f, dmax = 0.f;
    for (int v = 0; v < V; v++) focal_max = r3::fmax_(focal_max, cams[r3::kMipCamFloats * v + 16]);
    for (int i = 0; i < n; i++) {
        float d = 0.f;
        for (int v = 0; v < V; v++) {
            const float z = r3::mip_filter_valid(cams + r3::kMipCamFloats * v, means + 3 * i);
            if (z > 0.f) d = d > 0.f ? r3::fmin_(d, z) : z;
        }
        filter[i] = d > 0.f ? r3::mip_filter_value(d, focal_max) : -1.f;
        dmax = r3::fmax_(dmax, d);
    }
    const float fill = dmax > 0.f ? r3::mip_filter_value(dmax, focal_max) : 0.f;
    for (int i = 0; i < n; i++)
        if (filter[i] < 0.f) filter[i] = fill;
}

void hc_mip_filtered(int n, const float* ls, const float* o, const float* f, float* ls_eff, float* raw_eff)
{
    for (int i = 0; i < n; i++) r3::mip_filtered_one(ls + 3 * i, o[i], f[i], ls_eff + 3 * i, raw_eff + i);
}

void hc_mip_filtered_bwd(int n, const float* ls, const float* o, const float* f, const float* g_ls, const float* g_o, float* d_ls,
                         float* d_o)
{
    for (int i = 0; i < n; i++) r3::mip_filtered_bwd_one(ls + 3 * i, o[i], f[i], g_ls + 3 * i, g_o[i], d_ls + 3 * i, d_o + i);
}

// cov2d of the forward with its dilation taken off again, against the undilated double covariance: (a + 0.3f, b, c + 0.3f)
// as gauss_math.h forms them, and (a, b, c) as mip_math.h does, for one Gaussian (activated scale / rotation)
void hc_mip_cov2d_both(const float* mean, const float* scale, const float* q, const float* view, float tan_fovx, float tan_fovy, int W,
                       int H, float mod, float* fwd3, double* mip3)
{
    r3::Camera cam{};
    for (int k = 0; k < 16; k++) cam.view[k] = view[k];
    cam.tan_fovx = tan_fovx;
    cam.tan_fovy = tan_fovy;
    cam.focal_x = W / (2.0f * tan_fovx);
    cam.focal_y = H / (2.0f * tan_fovy);
    cam.scale_modifier = mod;
    float c6[6], A[6], t[3], xm, ym;
    r3::cov3d_from_scale_rot(scale, mod, q, c6);
    r3::ewa_A(cam, mean[0], mean[1], mean[2], A, t, &xm, &ym);
    r3::cov2d(A, c6, fwd3, fwd3 + 1, fwd3 + 2);
    const r3::MipView v = r3::mip_make_view(view, tan_fovx, tan_fovy, W, H, mod);
    float tf[3];
    r3::xform4x3(view, mean[0], mean[1], mean[2], tf);
    r3::MipCov C;
    r3::mip_cov3d(scale, mod, q, C.S6);
    r3::mip_cov2d(v, mean, tf, C);
    mip3[0] = C.a;
    mip3[1] = C.b;
    mip3[2] = C.c;
}

}  // extern "C"

#ifdef HOSTCHECK_MIP_MAIN
// Every function over its edge inputs; prints a checksum so that nothing is optimised away.  Exit status 1 on a broken
// invariant (a non-finite value or gradient where one must be finite, f == 0 not returning its inputs).
int main()
{
    int bad = 0;
    double sum = 0.0;
    const int n = 600, V = 70;
    std::vector<float> means(3 * n), sc(3 * n), rot(4 * n), op(n), cov(6 * n), out(n), rho(n), g(n, 1.f), d_o(n), dm(3 * n), ds(3 * n),
        dq(4 * n), dc(6 * n), cams(20 * V), filt(n), ls_eff(3 * n), d_ls(3 * n);
    const float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.1f, -0.2f, 3.f, 1};
    for (int i = 0; i < n; i++) {
        means[3 * i] = -2.f + 0.007f * i;
        means[3 * i + 1] = 1.f - 0.004f * i;
        means[3 * i + 2] = i % 10 == 0 ? -3.5f : -1.f + 0.01f * i;   // a tenth behind the near plane
        op[i] = -15.f + 0.05f * i;
        for (int k = 0; k < 3; k++) sc[3 * i + k] = i % 10 == 1 ? (k ? -9.f : -2.f) : (i % 10 == 2 ? -11.f : -4.f + 0.3f * k);
        for (int k = 0; k < 4; k++) rot[4 * i + k] = i == 5 ? 0.f : (0.3f + k) * (k % 2 ? -1.f : 1.f) * (i % 3 ? 1.f : 1e-3f);
    }
    for (int raw = 1; raw >= 0; raw--) {
        if (!raw)   // activated inputs for the second round
            for (int i = 0; i < n; i++) {
                float q[4];
                r3::quat_act(&rot[4 * i], q);
                for (int k = 0; k < 4; k++) rot[4 * i + k] = q[k];
                for (int k = 0; k < 3; k++) sc[3 * i + k] = r3::scale_act(sc[3 * i + k]);
            }
        hc_mip_opacity(n, means.data(), sc.data(), rot.data(), nullptr, op.data(), raw, view, 0.6f, 0.45f, 64, 48, 1.f, out.data(),
                       rho.data());
        hc_mip_opacity_bwd(n, means.data(), sc.data(), rot.data(), nullptr, op.data(), raw, view, 0.6f, 0.45f, 64, 48, 1.f, g.data(),
                           d_o.data(), dm.data(), ds.data(), dq.data(), dc.data());
        for (int i = 0; i < n; i++) {
            bad += !std::isfinite(out[i]) || !(rho[i] >= 0.005f && rho[i] <= 1.f) || !std::isfinite(d_o[i]);
            for (int k = 0; k < 3; k++) bad += !std::isfinite(dm[3 * i + k]) || !std::isfinite(ds[3 * i + k]);
            for (int k = 0; k < 4; k++) bad += !std::isfinite(dq[4 * i + k]);
            sum += out[i] + rho[i] + d_o[i] + dm[3 * i] + ds[3 * i] + dq[4 * i];
        }
    }
    for (int i = 0; i < n; i++) {
        const float c6[6] = {0.01f, 0.001f, 0.f, 0.02f, 0.002f, 0.0001f * (i % 7)};
        for (int k = 0; k < 6; k++) cov[6 * i + k] = c6[k];
    }
    hc_mip_opacity(n, means.data(), nullptr, nullptr, cov.data(), op.data(), 0, view, 0.6f, 0.45f, 64, 48, 1.f, out.data(), rho.data());
    hc_mip_opacity_bwd(n, means.data(), nullptr, nullptr, cov.data(), op.data(), 0, view, 0.6f, 0.45f, 64, 48, 1.f, g.data(), d_o.data(),
                       dm.data(), ds.data(), dq.data(), dc.data());
    for (int i = 0; i < n; i++) {
        bad += !std::isfinite(out[i]) || !std::isfinite(dc[6 * i]) || !std::isfinite(dc[6 * i + 5]);
        sum += out[i] + dc[6 * i + 1];
    }
    for (int v = 0; v < V; v++) {
        for (int k = 0; k < 16; k++) cams[20 * v + k] = view[k];
        cams[20 * v + 14] = 2.f + 0.05f * v;
        cams[20 * v + 16] = 50.f + v;
        cams[20 * v + 17] = 40.f + v;
        cams[20 * v + 18] = 64.f;
        cams[20 * v + 19] = 48.f;
    }
    hc_mip_filter3d(n, V, means.data(), cams.data(), filt.data());
    for (int i = 0; i < n; i++) {
        bad += !(filt[i] >= 0.f) || !std::isfinite(filt[i]);
        sum += filt[i];
    }
    hc_mip_filter3d(n, 0, means.data(), cams.data(), filt.data());
    for (int i = 0; i < n; i++) bad += filt[i] != 0.f;
    for (int i = 0; i < n; i++) filt[i] = i % 4 ? 0.001f * i : 0.f;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) sc[3 * i + k] = -12.f + 0.02f * i + k;
    hc_mip_filtered(n, sc.data(), op.data(), filt.data(), ls_eff.data(), out.data());
    hc_mip_filtered_bwd(n, sc.data(), op.data(), filt.data(), ds.data(), g.data(), d_ls.data(), d_o.data());
    for (int i = 0; i < n; i++) {
        if (filt[i] == 0.f) bad += out[i] != op[i] || ls_eff[3 * i] != sc[3 * i] || d_o[i] != g[i] || d_ls[3 * i + 2] != ds[3 * i + 2];
        bad += !std::isfinite(out[i]) || !std::isfinite(ls_eff[3 * i + 1]) || !std::isfinite(d_o[i]) || !std::isfinite(d_ls[3 * i]);
        sum += out[i] + ls_eff[3 * i] + d_o[i] + d_ls[3 * i];
    }
    std::printf("checksum %.9g bad %d\n", sum, bad);
    return bad ? 1 : 0;
}
#endif
