// quant_math.h -- the quantised (codebook-indexed) model as the kernels read it: half -> float, where a Gaussian's ids
// sit, and the lookup, per element.  Shared by the quantised instantiations of the per-Gaussian kernels (preprocess.hip),
// by r3dgs_quantised_decode (capi.hip -> preprocess.hip) and by the CPU test shim tests/hostcheck_quant/hostcheck_quant.hip,
// so the exact source a lane executes is checked without a GPU.
//
// What it restates (scene/gaussian_model.py of the reference): save_ply(quantised=True) stores, per Gaussian and grouped by
// SH degree, one byte per attribute -- an index into one of twenty 256-entry codebooks -- and the position as float or
// half; load_ply looks every index up again (:371-387).  Nothing here rounds: a lookup copies a float, and every half is
// a float exactly.
//
// Device representation (include/r3dgs_quantised.h):
//   xyz        half [P,3] (bit pattern) or float [P,3]
//   geom_ids   uint8 [P,8]   opacity, scale x/y/z, rotation re, rotation im x/y/z
//   sh_ids     uint8, ragged: Gaussian i of degree d owns 3 (d+1)^2 bytes, [coefficient][channel], starting at byte
//              3 * quant_ragged_offset(i)
//   codebooks  float [20][256], rows in the file's order (QuantBook)
#ifndef R3DGS_QUANT_MATH_H
#define R3DGS_QUANT_MATH_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace r3 {

constexpr int kQuantBooks = 20;      // codebooks of a model
constexpr int kQuantCentres = 256;   // entries of each
constexpr int kQuantShBooks = 16;    // the first sixteen colour the Gaussians: book k serves SH coefficient k
enum QuantBook { kBookDc = 0, kBookRest0 = 1, kBookOpacity = 16, kBookScaling = 17, kBookRotRe = 18, kBookRotIm = 19 };

__host__ __device__ inline float quant_bits_to_float(uint32_t b)
{
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}

// IEEE binary16 bit pattern -> the float of the same value (exact for every input; NaN payloads keep their top bits).
// A subnormal half m * 2^-24 (m < 1024) is the product of two floats whose exact product is a normal float.
__host__ __device__ inline float quant_half_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 0) {
        const float mag = (float)m * 5.9604644775390625e-08f;   // m * 2^-24; +0 for m == 0
        return sign ? -mag : mag;                               // (-mag of +0 is -0)
    }
    if (e == 31) return quant_bits_to_float(sign | 0x7f800000u | (m << 13));
    return quant_bits_to_float(sign | ((e + 112u) << 23) | (m << 13));
}

// forward.cu:19-36 getSHOffset, in units of one coefficient (three ids): where Gaussian idx's SH row starts when the
// Gaussians are sorted by degree; *deg is its degree.  coeffs = {1, 4, 9, 16}, perband the Gaussians of each degree,
// cumsum their running sum.
__host__ __device__ inline int quant_ragged_offset(int idx, const int* coeffs, const int* perband, const int* cumsum, int* deg)
{
    int off = 0;
    *deg = 0;
    if (idx < cumsum[0]) return idx * coeffs[0];
    *deg = 1;
    off += perband[0] * coeffs[0];
    if (idx < cumsum[1]) return off + (idx - cumsum[0]) * coeffs[1];
    *deg = 2;
    off += perband[1] * coeffs[1];
    if (idx < cumsum[2]) return off + (idx - cumsum[1]) * coeffs[2];
    *deg = 3;
    off += perband[2] * coeffs[2];
    return off + (idx - cumsum[2]) * coeffs[3];
}

// bytes of sh_ids
__host__ __device__ inline long long quant_sh_bytes(const int* coeffs, const int* perband)
{
    long long n = 0;
    for (int d = 0; d < 4; d++) n += 3LL * perband[d] * coeffs[d];
    return n;
}

// codebook of element e = 3 * coefficient + channel of an SH row: features_dc for coefficient 0, features_rest_{k-1} for k
__host__ __device__ inline int quant_sh_book(int e) { return (int)(((uint32_t)e * 43691u) >> 17); }   // e / 3 for e < 2^15

__host__ __device__ inline float quant_lookup(const float* codebooks, int book, uint32_t id)
{
    return codebooks[book * kQuantCentres + (int)id];
}

__host__ __device__ inline void quant_xyz(const void* xyz, int xyz_is_half, long long i, float out[3])
{
    if (xyz_is_half) {
        const uint16_t* p = static_cast<const uint16_t*>(xyz) + 3 * i;
        out[0] = quant_half_to_float(p[0]);
        out[1] = quant_half_to_float(p[1]);
        out[2] = quant_half_to_float(p[2]);
    } else {
        const float* p = static_cast<const float*>(xyz) + 3 * i;
        out[0] = p[0];
        out[1] = p[1];
        out[2] = p[2];
    }
}

// The model's raw parameters of one Gaussian from its eight geometry ids (g[0..7], see above): opacity logit, log-scales,
// the quaternion as stored (re and im were quantised apart: not unit length).
__host__ __device__ inline void quant_geom(const float* codebooks, const uint8_t g[8], float* opacity, float scale[3], float rot[4])
{
    *opacity = quant_lookup(codebooks, kBookOpacity, g[0]);
    for (int k = 0; k < 3; k++) scale[k] = quant_lookup(codebooks, kBookScaling, g[1 + k]);
    rot[0] = quant_lookup(codebooks, kBookRotRe, g[4]);
    for (int k = 0; k < 3; k++) rot[1 + k] = quant_lookup(codebooks, kBookRotIm, g[5 + k]);
}

// One Gaussian's SH row as sh_to_rgb reads it: element e of the row whose ids start at `ids`.
struct ShRowQuantPlain {
    const uint8_t* ids;
    const float* codebooks;
    __host__ __device__ float at(int e) const { return quant_lookup(codebooks, quant_sh_book(e), ids[e]); }
};

// Everything the reference's load_ply returns for Gaussian i: _xyz [P,3], _features_dc [P,1,3], _features_rest [P,15,3],
// _opacity [P,1], _scaling [P,3], _rotation [P,4], _degrees [P,1].  Coefficients above the Gaussian's degree are not
// stored; the reference pads their INDEX with zero, so they decode to centre 0 of their codebook.  Any output may be null.
__host__ __device__ inline void quant_decode_one(int i, const int* coeffs, const int* perband, const int* cumsum, const void* xyz,
                                                 int xyz_is_half, const uint8_t* geom_ids, const uint8_t* sh_ids,
                                                 const float* codebooks, float* xyz_out, float* features_dc,
                                                 float* features_rest, float* opacity, float* scaling, float* rotation,
                                                 int* degrees)
{
    int deg;
    const long long off = 3LL * quant_ragged_offset(i, coeffs, perband, cumsum, &deg);
    const long long r = i;
    if (xyz_out) quant_xyz(xyz, xyz_is_half, r, xyz_out + 3 * r);
    float op, sc[3], q[4];
    quant_geom(codebooks, geom_ids + 8 * r, &op, sc, q);
    if (opacity) opacity[r] = op;
    if (scaling)
        for (int k = 0; k < 3; k++) scaling[3 * r + k] = sc[k];
    if (rotation)
        for (int k = 0; k < 4; k++) rotation[4 * r + k] = q[k];
    if (degrees) degrees[r] = deg;
    const ShRowQuantPlain row{sh_ids + off, codebooks};
    if (features_dc)
        for (int c = 0; c < 3; c++) features_dc[3 * r + c] = row.at(c);
    if (features_rest) {
        const int stored = 3 * (deg + 1) * (deg + 1);
        for (int e = 3; e < 48; e++)
            features_rest[45 * r + (e - 3)] = e < stored ? row.at(e) : quant_lookup(codebooks, quant_sh_book(e), 0u);
    }
}

// ---- the adjoint of the lookup (r3dgs_quantised_codebook_grad, quant_grad.hip) ------------------------------------------
// A Gaussian has kQuantSlots id slots: its 8 geometry ids, then the 48 elements of a full SH row, of which a Gaussian of
// degree d owns the first 3 (d+1)^2.  Slot s of Gaussian i adds one element of one of the five gradient tensors -- shaped as
// quant_decode_one writes its outputs -- to centre *id of codebook `book`.  This is the ONE statement of that mapping: the
// kernel and tests/hostcheck_quant_grad both call it.
constexpr int kQuantGeomSlots = 8;
constexpr int kQuantSlots = kQuantGeomSlots + 48;
enum QuantGradTensor { kGradDc = 0, kGradRest, kGradOpacity, kGradScaling, kGradRotation, kQuantGradTensors };

struct QuantGradSlot {
    int book;            // QuantBook row of dL_dcodebooks
    int tensor;          // QuantGradTensor
    long long elem;      // element of that tensor (flat index)
    const uint8_t* id;   // the byte that names the centre
};

// sh_off: the byte of sh_ids at which Gaussian i's row starts, 3 * quant_ragged_offset(i); deg its degree.  False for an SH
// slot above the degree: the decoder pads those with centre 0, nobody owns them, and their gradient is not read.
__host__ __device__ inline bool quant_grad_slot(int s, long long i, int deg, long long sh_off, const uint8_t* geom_ids,
                                                const uint8_t* sh_ids, QuantGradSlot* o)
{
    if (s < kQuantGeomSlots) {
        o->id = geom_ids + 8 * i + s;
        if (s == 0) {
            o->book = kBookOpacity, o->tensor = kGradOpacity, o->elem = i;
        } else if (s < 4) {
            o->book = kBookScaling, o->tensor = kGradScaling, o->elem = 3 * i + (s - 1);
        } else {
            o->book = s == 4 ? kBookRotRe : kBookRotIm, o->tensor = kGradRotation, o->elem = 4 * i + (s - 4);
        }
        return true;
    }
    const int e = s - kQuantGeomSlots;   // element of the SH row: 3 * coefficient + channel
    if (e >= 3 * (deg + 1) * (deg + 1)) return false;
    o->id = sh_ids + sh_off + e;
    o->book = quant_sh_book(e);
    if (e < 3) {
        o->tensor = kGradDc, o->elem = 3 * i + e;
    } else {
        o->tensor = kGradRest, o->elem = 45 * i + (e - 3);
    }
    return true;
}

// The reduction's shape, a function of P alone (never of the device): a chunk is kQuantGradChunk consecutive Gaussians; a
// group is a run of consecutive chunks that one wave sums into one partial table; at most kQuantGradMaxGroups groups.
constexpr int kQuantGradChunk = 1024;
constexpr int kQuantGradMaxGroups = 2048;

__host__ __device__ inline int quant_grad_chunks(int P) { return (int)(((long long)P + kQuantGradChunk - 1) / kQuantGradChunk); }
__host__ __device__ inline int quant_grad_chunks_per_group(int P)
{
    const int c = quant_grad_chunks(P);
    return c <= kQuantGradMaxGroups ? 1 : (c + kQuantGradMaxGroups - 1) / kQuantGradMaxGroups;
}
__host__ __device__ inline int quant_grad_groups(int P)
{
    const int c = quant_grad_chunks(P), per = quant_grad_chunks_per_group(P);
    return (c + per - 1) / per;
}

// resident bytes of a model (the band tables: three int[4])
__host__ __device__ inline long long quant_model_bytes(long long P, const int* perband, int xyz_is_half)
{
    long long n = P * (8 + (xyz_is_half ? 6 : 12)) + (long long)kQuantBooks * kQuantCentres * 4 + 3 * 4 * 4;
    for (int d = 0; d < 4; d++) n += 3LL * (d + 1) * (d + 1) * perband[d];
    return n;
}

}  // namespace r3

#endif  // R3DGS_QUANT_MATH_H
