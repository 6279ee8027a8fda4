// hostcheck_densify.hip -- TEST SHIM: runs the product's per-Gaussian densification arithmetic (reduced-3dgs_amd/csrc/
// densify_math.h, the __host__ __device__ functions csrc/densify.hip executes per lane) on the CPU, so
// tests/test_densify_cpu.py can compare it with the numpy restatement WITHOUT a GPU.  Not part of the product; nothing in
// reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/densify_math.h"

extern "C" {

// plan_kernel's per-lane body for n Gaussians
void hc_densify_flags(int n, int densify, float max_grad, float dense_scale, float min_opacity, int screen, float max_screen,
                      float world_scale, const float* accum, const float* denom, const float* scaling, const float* opacity,
                      const float* max_radii, unsigned char* flags)
{
    r3::DensifyThresholds t;
    t.max_grad = max_grad;
    t.dense_scale = dense_scale;
    t.min_opacity = min_opacity;
    t.max_screen = max_screen;
    t.world_scale = world_scale;
    t.densify = densify;
    t.screen = screen;
    for (int i = 0; i < n; i++) flags[i] = r3::densify_flags(t, accum[i], denom[i], scaling + 3 * i, opacity[i], max_radii[i]);
}

void hc_densify_grad(int n, const float* accum, const float* denom, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::densify_grad(accum[i], denom[i]);
}

void hc_scale_act(int n, const float* raw, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::scale_act(raw[i]);
}

void hc_child_scaling(int n, const float* scale, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::child_scaling(scale[i]);
}

// new_row_word's XYZ branch: raw_q [n,4], scale [n,3] (activated), noise [n,3], xyz [n,3] -> out [n,3]
void hc_child_xyz(int n, const float* raw_q, const float* scale, const float* noise, const float* xyz, float* out)
{
    for (int i = 0; i < n; i++)
        for (int w = 0; w < 3; w++) out[3 * i + w] = r3::child_xyz(w, raw_q + 4 * i, scale + 3 * i, noise + 3 * i, xyz[3 * i + w]);
}

}  // extern "C"
