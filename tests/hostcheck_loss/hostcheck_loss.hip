// hostcheck_loss.hip -- TEST SHIM: runs the product's per-pixel loss arithmetic (reduced-3dgs_amd/csrc/loss_math.h, the
// __host__ __device__ functions csrc/loss.hip executes per lane) on the CPU, so tests/test_loss_cpu.py can compare it with
// a float64 evaluation WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/loss_math.h"

extern "C" {

// out[4 i + 0..3] = S, dS/dmu_x, dS/dE_xx, dS/dE_xy of the moments (mx, my, exx, eyy, exy)[i]
void hc_ssim_pixel(int n, const float* mx, const float* my, const float* exx, const float* eyy, const float* exy, float* out)
{
    for (int i = 0; i < n; i++) {
        const r3::SsimPixel p = r3::ssim_pixel(mx[i], my[i], exx[i], eyy[i], exy[i]);
        out[4 * i] = p.s;
        out[4 * i + 1] = p.d_mu;
        out[4 * i + 2] = p.d_exx;
        out[4 * i + 3] = p.d_exy;
    }
}

void hc_l1_sign(int n, const float* x, const float* y, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::l1_sign(x[i], y[i]);
}

float hc_ssim_c1(void) { return r3::kSsimC1; }
float hc_ssim_c2(void) { return r3::kSsimC2; }

}  // extern "C"
