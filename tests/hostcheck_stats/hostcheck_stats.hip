// hostcheck_stats.hip -- TEST SHIM: runs the product's per-element training-statistics arithmetic (reduced-3dgs_amd/csrc/
// stats_math.h, the __host__ __device__ functions csrc/train_stats.hip executes per lane) on the CPU, so
// tests/test_train_stats_cpu.py can compare it with the numpy restatement WITHOUT a GPU.  Not part of the product; nothing in
// reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/stats_math.h"

extern "C" {

// densification_stats_kernel's body for n Gaussians, in place: a culled Gaussian's gradient row is not read
void hc_densification_stats(int n, const float* vg, const int* radii, float* grad_accum, float* denom, float* max_radii)
{
    for (int i = 0; i < n; i++) {
        float gx = 0.f, gy = 0.f;
        if (radii[i] > 0) {
            gx = vg[3 * i];
            gy = vg[3 * i + 1];
        }
        r3::densify_update(radii[i], gx, gy, grad_accum[i], denom[i], max_radii[i]);
    }
}

void hc_sigmoid(int n, const float* x, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::stats_sigmoid(x[i]);
}

void hc_sigmoid_grad(int n, const float* x, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::stats_sigmoid_grad(x[i]);
}

void hc_alpha_regul_term(int n, const float* x, float scale, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::alpha_regul_term(x[i], scale);
}

}  // extern "C"
