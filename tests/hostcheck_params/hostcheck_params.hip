// hostcheck_params.hip -- TEST SHIM: runs the product's activation arithmetic (reduced-3dgs_amd/csrc/param_math.h, the
// __host__ __device__ functions the raw-parameter kernels execute per lane) on the CPU, so tests/test_params_cpu.py can hold
// it to float64 WITHOUT a GPU, and tests/test_params_gpu.py can restate the kernels' activation backward bit for bit.
// Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/param_math.h"

extern "C" {

void hc_scale_act(int n, const float* raw, float* s)
{
    for (int i = 0; i < n; i++) s[i] = r3::scale_act(raw[i]);
}

void hc_scale_act_bwd(int n, const float* g, const float* s, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::scale_act_bwd(g[i], s[i]);
}

// raw, q: [n][4]; norm: [n]
void hc_quat_act(int n, const float* raw, float* q, float* norm)
{
    for (int i = 0; i < n; i++) norm[i] = r3::quat_act(raw + 4 * i, q + 4 * i);
}

void hc_quat_act_bwd(int n, const float* q, const float* norm, const float* g, float* out)
{
    for (int i = 0; i < n; i++) r3::quat_act_bwd(q + 4 * i, norm[i], g + 4 * i, out + 4 * i);
}

// the header's own error bounds (doubles): scale [n], rotation [n][4]
void hc_scale_act_bwd_bound(int n, const double* g, const double* s, double exp_ulps, double* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::scale_act_bwd_bound(g[i], s[i], exp_ulps);
}

void hc_quat_act_bwd_bound(int n, const double* q, const double* norm, const double* g, double* out)
{
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 4; k++) out[4 * i + k] = r3::quat_act_bwd_bound(q + 4 * i, norm[i], g + 4 * i, k);
}

float hc_normalize_eps(void) { return r3::kNormalizeEps; }

}  // extern "C"
