// hostcheck_optim.hip -- TEST SHIM: runs the product's per-element Adam arithmetic (reduced-3dgs_amd/csrc/adam_math.h, the
// __host__ __device__ function csrc/optim.hip executes per lane) on the CPU, so tests/test_optim_cpu.py can compare it with
// a float32 restatement bit for bit WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/adam_math.h"

extern "C" {

// One step of n elements in place; s[6] = w1, beta2, w2, bc2_sqrt, eps, step_size (r3::AdamScalars)
void hc_adam_step(int n, const float* s, const float* g, float* p, float* m, float* v)
{
    const r3::AdamScalars sc{s[0], s[1], s[2], s[3], s[4], s[5]};
    for (int i = 0; i < n; i++) r3::adam_element(sc, g[i], p[i], m[i], v[i]);
}

}  // extern "C"
