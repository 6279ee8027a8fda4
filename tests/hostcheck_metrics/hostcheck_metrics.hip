// hostcheck_metrics.hip -- TEST SHIM: runs the product's per-sample metric arithmetic (reduced-3dgs_amd/csrc/metrics_math.h,
// the __host__ __device__ functions csrc/metrics.hip executes per lane) on the CPU, so tests/test_metrics_cpu.py can compare
// it with torch's CPU results bit for bit WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/metrics_math.h"

extern "C" {

void hc_quantise8(int n, const float* x, unsigned char* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::metrics_quantise8(x[i]);
}

void hc_load_u8(int n, const unsigned char* u, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::metrics_load(u[i], 0);
}

void hc_load_f32(int n, const float* x, int flags, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::metrics_load(x[i], flags);
}

void hc_err(int n, const float* x, const float* y, double* abs_err, double* sq_err)
{
    for (int i = 0; i < n; i++) {
        abs_err[i] = r3::metrics_abs_err(x[i], y[i]);
        sq_err[i] = r3::metrics_sq_err(x[i], y[i]);
    }
}

}  // extern "C"
