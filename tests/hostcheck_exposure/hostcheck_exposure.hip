// hostcheck_exposure.hip -- TEST SHIM: runs the product's per-pixel exposure arithmetic (reduced-3dgs_amd/csrc/exposure_math.h,
// the __host__ __device__ functions the exposure kernels of csrc/loss.hip execute per lane) on the CPU, so
// tests/test_exposure_loss_cpu.py can compare it with a float64 evaluation WITHOUT a GPU.  Not part of the product; nothing in
// reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/exposure_math.h"

extern "C" {

// out[3 i + c] = x''_c of pixel i: E[12 i ..] its exposure, x[3 i ..] its three channels, m[i] its mask weight
void hc_exposed(int n, const float* E, const float* x, const float* m, float* out)
{
    for (int i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) out[3 * i + c] = r3::exposed(E + 12 * i, x[3 * i], x[3 * i + 1], x[3 * i + 2], m[i], c);
}

// out[3 i + k] = dx_k of pixel i for the upstream gradient g[3 i ..] of x''
void hc_exposed_adjoint(int n, const float* E, const float* g, const float* m, float* out)
{
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) out[3 * i + k] = r3::exposed_adjoint(E + 12 * i, g[3 * i], g[3 * i + 1], g[3 * i + 2], m[i], k);
}

// out[12 i ..] = the twelve terms pixel i adds to dE (each pixel into its own zeroed accumulator)
void hc_exposure_grad_terms(int n, const float* x, const float* g, const float* m, double* out)
{
    for (int i = 0; i < n; i++) {
        double dE[r3::kExposureFloats] = {0.0};
        r3::exposure_grad_accumulate(dE, x[3 * i], x[3 * i + 1], x[3 * i + 2], g[3 * i], g[3 * i + 1], g[3 * i + 2], m[i]);
        for (int j = 0; j < r3::kExposureFloats; j++) out[12 * i + j] = dE[j];
    }
}

}  // extern "C"
