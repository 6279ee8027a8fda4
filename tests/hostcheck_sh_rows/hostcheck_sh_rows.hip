// hostcheck_sh_rows.hip -- TEST SHIM: the __host__ __device__ index functions of reduced-3dgs_amd/csrc/sh_rows.h (where an
// element of a wave's SH span sits in the LDS window) on the CPU, so tests/test_sh_rows_cpu.py can check the layout and its
// multiply-and-shift divisions exhaustively WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/sh_rows.h"

extern "C" {

int hs_row_floats() { return r3::kShRowFloats; }
int hs_window_floats() { return r3::kWaveShFloats; }

// out[e] = sh_skew<rows48>(first + e)
void hs_skew(int rows48, int first, int n, int* out)
{
    for (int e = 0; e < n; e++) out[e] = rows48 ? r3::sh_skew<true>(first + e) : r3::sh_skew<false>(first + e);
}

// out[f] = sh_split_index<rows48>(f, rl, k0, M)
void hs_split_index(int rows48, int n, int rl, int k0, int M, int* out)
{
    for (int f = 0; f < n; f++) out[f] = rows48 ? r3::sh_split_index<true>(f, rl, k0, M) : r3::sh_split_index<false>(f, rl, k0, M);
}

}  // extern "C"
