// adam_math.h -- per-element arithmetic of the fused Adam step (optim.hip), shared with the CPU test shim
// tests/hostcheck_optim/hostcheck_optim.hip so the exact source the kernel executes per lane is checked without a GPU.
//
// It reproduces torch.optim.Adam's default (foreach) step for fp32 tensors with amsgrad, maximize, weight_decay and
// capturable all off, op for op and rounding for rounding.  That step is five elementwise passes per tensor list:
//   m <- lerp(m, g, 1 - beta1)
//   v <- v * beta2
//   v <- addcmul(v, g, g, value = 1 - beta2)
//   d <- sqrt(v) / bc2_sqrt + eps
//   p <- addcdiv(p, m, d, value = step_size)
// with host scalars computed in Python doubles (step: the count after this step's bump)
//   bc1 = 1 - beta1**step,  bc2 = 1 - beta2**step,  step_size = -(lr / bc1),  bc2_sqrt = bc2**0.5
// and each rounded to fp32 once on its way into the kernel, as are 1 - beta1, beta2, 1 - beta2 and eps (AdamScalars).
//
// Where torch's ROCm build rounds was settled on an MI355X against torch 2.10 (ROCm 7.0) on the same inputs, one sweep
// over the sixteen variants {lerp, addcmul, addcdiv: one fma or a rounded product and sum} x {divide by bc2_sqrt or
// multiply by its reciprocal}: only the variant written here reproduces torch's p, m and v bit for bit.
// Each line below names its roundings.  optim.hip is compiled with -ffp-contract=off and correctly rounded fp32 divide
// and sqrt, so the compiler adds and removes none: the fmas are explicit (__fmaf_rn on the device, fmaf on the host).
#ifndef R3DGS_ADAM_MATH_H
#define R3DGS_ADAM_MATH_H

#include <hip/hip_runtime.h>

#include <cmath>

namespace r3 {

// The fp32 scalars of one tensor's step.  Each is a double of the host (or of the capturable kernel) rounded once.
struct AdamScalars {
    float w1;          // 1 - beta1, the lerp weight
    float beta2;
    float w2;          // 1 - beta2, the addcmul value
    float bc2_sqrt;    // (1 - beta2**step) ** 0.5
    float eps;
    float step_size;   // -(lr / (1 - beta1**step))
};

__host__ __device__ inline float adam_fma(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return std::fma(a, b, c);
#endif
}

// One element: updates p, m, v in place.
__host__ __device__ inline void adam_element(const AdamScalars& s, float g, float& p, float& m, float& v)
{
    // lerp(m, g, w1) -- torch takes the form with the smaller weight: m + w1 (g - m) for w1 < 0.5, else
    // g - (g - m)(1 - w1); the difference and (1 - w1) rounded, then one fma
    const float dg = g - m;                                                              // 1 rounding
    m = s.w1 < 0.5f ? adam_fma(s.w1, dg, m)                                              // 1 rounding (fma)
                    : adam_fma(-dg, 1.0f - s.w1, g);                                     // 2 roundings (1 - w1, fma)
    v = v * s.beta2;                                                                     // 1 rounding
    v = adam_fma(s.w2, g * g, v);                                                        // 2 roundings (g g, fma)
    const float d = std::sqrt(v) / s.bc2_sqrt + s.eps;                                   // 3 roundings (sqrt, /, +)
    p = adam_fma(s.step_size, m / d, p);                                                 // 2 roundings (m / d, fma)
}

// ---- the visibility-gated step (optim.hip's adam_visible_kernel): a tensor is [P, row_len] floats, element e belongs to
// Gaussian e / row_len, and only Gaussians with radii > 0 are updated.  A workgroup divides once, uniformly (chunk_origin:
// the Gaussian and the remainder of its chunk's first element); its lanes then divide 32-bit offsets from there by a
// multiply-high with the row's reciprocal and one fix-up (row_divmod), and walk the other three elements of a float4.

// floor(2^32 / len) of a row (len >= 1; len == 1 takes 2^32 - 1: the fix-up below covers it).
struct RowDiv {
    unsigned len;
    unsigned magic;
};

__host__ __device__ inline RowDiv row_div(int row_len)
{
    const unsigned len = (unsigned)row_len;
    return {len, len == 1 ? 0xffffffffu : (unsigned)(0x100000000ull / len)};
}

__host__ __device__ inline unsigned mulhi_u32(unsigned a, unsigned b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}

// x / len with the remainder, for any 32-bit x: the multiply-high is the quotient or one less.
__host__ __device__ inline unsigned row_divmod(const RowDiv& d, unsigned x, unsigned& rem)
{
    unsigned q = mulhi_u32(x, d.magic);
    rem = x - q * d.len;
    if (rem >= d.len) {
        rem -= d.len;
        q++;
    }
    return q;
}

// Where a chunk starts: element e0 of the tensor lies in Gaussian `gaussian`, `rem` floats into its row.
struct ChunkOrigin {
    long long gaussian;
    unsigned rem;
};

__host__ __device__ inline ChunkOrigin chunk_origin(const RowDiv& d, long long e0)
{
    ChunkOrigin o;
    if ((unsigned long long)e0 >> 32 == 0) {
        o.gaussian = row_divmod(d, (unsigned)e0, o.rem);
    } else {   // past 2^32 elements: one 64-bit division per workgroup
        o.gaussian = e0 / (long long)d.len;
        o.rem = (unsigned)(e0 - o.gaussian * (long long)d.len);
    }
    return o;
}

// The Gaussian, counted from the chunk's origin, of the element `offset` floats after the chunk's first one
// (offset < 2^31, so rem + offset fits 32 bits for any int row_len).
__host__ __device__ inline unsigned element_gaussian(const RowDiv& d, unsigned origin_rem, unsigned offset, unsigned& rem)
{
    return row_divmod(d, origin_rem + offset, rem);
}

// The Gaussians of the four consecutive elements that start `offset` floats after the chunk's first one: at most
// min(4, ceil(3 / len) + 1) different ones, q[0] <= q[1] <= q[2] <= q[3].
__host__ __device__ inline void unit_gaussians(const RowDiv& d, unsigned origin_rem, unsigned offset, unsigned q[4])
{
    unsigned rem;
    q[0] = element_gaussian(d, origin_rem, offset, rem);
#pragma unroll
    for (int j = 1; j < 4; j++) {
        rem++;
        const bool next = rem == d.len;
        rem = next ? 0u : rem;
        q[j] = q[j - 1] + (next ? 1u : 0u);
    }
}

// The Gaussian of the k-th element from the end of a [P, len] tensor (k = 0: the last one): the tail of a vector row.
__host__ __device__ inline long long tail_gaussian(const RowDiv& d, long long P, unsigned k)
{
    unsigned rem;
    return P - 1 - (long long)row_divmod(d, k, rem);
}

__host__ __device__ inline bool gaussian_visible(int radius) { return radius > 0; }

// One element of the gated step: adam_element where the Gaussian is visible; elsewhere p, m and v keep their bits and g is
// not looked at (a select, so that a NaN or Inf gradient of a culled row reaches nothing).
__host__ __device__ inline void adam_element_gated(const AdamScalars& s, bool visible, float g, float& p, float& m, float& v)
{
    float p1 = p, m1 = m, v1 = v;
    adam_element(s, g, p1, m1, v1);
    p = visible ? p1 : p;
    m = visible ? m1 : m;
    v = visible ? v1 : v;
}

}  // namespace r3

#endif  // R3DGS_ADAM_MATH_H
