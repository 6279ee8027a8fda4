// hostcheck_quant.hip -- TEST SHIM: runs the product's quantised-model arithmetic (reduced-3dgs_amd/csrc/quant_math.h, the
// __host__ __device__ functions the quantised kernels and r3dgs_quantised_decode execute per lane) on the CPU, so
// tests/test_quantised_cpu.py can hold the addressing, the row order and the half conversion to a numpy restatement
// WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/quant_math.h"

extern "C" {

void hq_half_to_float(int n, const uint16_t* h, float* out)
{
    for (int i = 0; i < n; i++) out[i] = r3::quant_half_to_float(h[i]);
}

// offsets [P] (in coefficients), degrees [P]
void hq_ragged_offsets(int P, const int* coeffs, const int* perband, const int* cumsum, int* offsets, int* degrees)
{
    for (int i = 0; i < P; i++) offsets[i] = r3::quant_ragged_offset(i, coeffs, perband, cumsum, degrees + i);
}

long long hq_sh_bytes(const int* coeffs, const int* perband) { return r3::quant_sh_bytes(coeffs, perband); }

long long hq_model_bytes(long long P, const int* perband, int xyz_is_half) { return r3::quant_model_bytes(P, perband, xyz_is_half); }

// r3dgs_quantised_decode on the host: the same per-Gaussian function
void hq_decode(int P, const int* coeffs, const int* perband, const int* cumsum, const void* xyz, int xyz_is_half,
               const uint8_t* geom_ids, const uint8_t* sh_ids, const float* codebooks, float* xyz_out, float* features_dc,
               float* features_rest, float* opacity, float* scaling, float* rotation, int* degrees)
{
    for (int i = 0; i < P; i++)
        r3::quant_decode_one(i, coeffs, perband, cumsum, xyz, xyz_is_half, geom_ids, sh_ids, codebooks, xyz_out, features_dc,
                             features_rest, opacity, scaling, rotation, degrees);
}

// the SH row of Gaussian i as the colour kernel's accessor hands it to sh_to_rgb: row[0 .. 3 (deg+1)^2)
int hq_sh_row(int i, const int* coeffs, const int* perband, const int* cumsum, const uint8_t* sh_ids, const float* codebooks,
              float* row)
{
    int deg;
    const long long off = 3LL * r3::quant_ragged_offset(i, coeffs, perband, cumsum, &deg);
    const r3::ShRowQuantPlain r{sh_ids + off, codebooks};
    for (int e = 0; e < 3 * (deg + 1) * (deg + 1); e++) row[e] = r.at(e);
    return deg;
}

}  // extern "C"
