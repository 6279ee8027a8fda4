// sh_rows.h -- how a wave's 64 SH rows lie in LDS, and the copies into and out of that layout.
//
// The per-Gaussian kernels that read SH rows (the forward's colour role in preprocess.hip, preprocess_bwd_kernel,
// colour_variance_accumulate_kernel) give each wave one LDS window.  The wave's 64 rows are one contiguous span of the
// [P,M,3] tensor (or of the ragged buffer, or one span of each of features_dc / features_rest): the wave copies it into
// the window with coalesced accesses, then every lane works on "element e of my row" through an accessor -- the interface
// of sh_to_rgb / sh_dir_derivs_at / sh_backward / sh_truncated_colours (gauss_math.h) -- and the backward copies the
// rows, rebuilt in place as gradient rows, out again the same way.  The lanes of a wave touch the same element of 64
// different rows, so the rows must start in different banks: the window is skewed.
//   ROWS48 (rows of 48 floats: every dense degree-3 tensor, M == 16): one word of padding per row, rows 49 words apart.
//     Element e of the lane's row is base[49 * lane + e] and e folds into the instruction's offset field: no address
//     arithmetic per access (the general scheme spent 30 % of the backward's vector instructions on it).
//   otherwise (ragged rows, other M): one word of padding per 32, the address is computed per access.
// Integer index arithmetic and copies only, no floating-point operation: the includers' contraction and rounding flags do
// not reach in here.  The index functions are __host__ __device__ and checked exhaustively on the CPU
// (tests/test_sh_rows_cpu.py).  Pointers are template parameters: a caller that works in the global address space
// (common.h global_ptr) passes such pointers and gets global loads and stores, a caller with plain pointers gets FLAT ones.
#ifndef R3DGS_SH_ROWS_H
#define R3DGS_SH_ROWS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace r3 {

constexpr int kShRowFloats = 48;                                              // the longest row: 16 coefficients x 3 channels
constexpr int kWaveShFloats = 64 * kShRowFloats + (64 * kShRowFloats) / 32;   // a wave's window: 64 rows + bank skew (3168)

// where float e of the wave's span (row after row) sits in the window
template <bool ROWS48>
__host__ __device__ __forceinline__ int sh_skew(int e)
{
    if (ROWS48) return e + (int)(((uint32_t)e * 43691u) >> 21);   // e + e / 48 for e < 2^16
    return e + (e >> 5);
}

// SH rows that arrive as two tensors (features_dc [P,1,3], features_rest [P,M-1,3]): the wave's 64 rows are one contiguous
// span of EACH, and both are copied into the one window layout, so that everything behind the staging is untouched.
// Float f of a span whose rows are `rl` floats long (3 for dc, 3 (M - 1) for rest) and start at float `k0` of the joined
// row (0 / 3) belongs to row f / rl: it is joined-span element row * 3M + k0 + f % rl.
// ROWS48: window word 49 * row + k0 + f % rl = f + (49 - rl) * row + k0 -- one multiply-high per float.
template <bool ROWS48>
__host__ __device__ __forceinline__ int sh_split_index(int f, int rl, int k0, int M)
{
    if (ROWS48) {   // rl is 3 or 45 (k0 says which): f / 3 and f / 45 for f < 2^16 by multiply and shift
        const int row = k0 == 0 ? (int)(((uint32_t)f * 43691u) >> 17) : (int)(((uint32_t)f * 46604u) >> 21);
        return f + (49 - rl) * row + k0;
    }
    const int row = f / rl;
    return sh_skew<false>(row * 3 * M + k0 + (f - row * rl));
}

// A lane's row.  F is float (at and put) or const float (at).
template <bool ROWS48, class F>
struct ShRow {
    F* base;    // ROWS48: the lane's row (window + 49 * lane); else the wave's window
    int roff;   // ROWS48: 0; else first float of the lane's row in the span
    __device__ __forceinline__ float at(int e) const { return ROWS48 ? base[e] : base[sh_skew<false>(roff + e)]; }
    __device__ __forceinline__ void put(int e, float v) const
    {
        if (ROWS48)
            base[e] = v;
        else
            base[sh_skew<false>(roff + e)] = v;
    }
};

// the row of `lane` in `window`; roff (its first float in the span) is lane * 3M for a dense tensor and matters only without ROWS48
template <bool ROWS48, class F>
__device__ __forceinline__ ShRow<ROWS48, F> sh_row(F* window, int lane, int roff)
{
    return {ROWS48 ? window + 49 * lane : window, ROWS48 ? 0 : roff};
}

// the float4 view of a span, in the span's own address space
__device__ __forceinline__ const float4* as_float4(const float* p) { return reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4* as_float4(float* p) { return reinterpret_cast<float4*>(p); }
#if defined(__HIP_DEVICE_COMPILE__)   // (the host pass knows no address spaces: these would repeat the two above)
#define R3_SH_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ const R3_SH_GLOBAL float4* as_float4(const R3_SH_GLOBAL float* p)
{
    return reinterpret_cast<const R3_SH_GLOBAL float4*>(p);
}
__device__ __forceinline__ R3_SH_GLOBAL float4* as_float4(R3_SH_GLOBAL float* p) { return reinterpret_cast<R3_SH_GLOBAL float4*>(p); }
#undef R3_SH_GLOBAL
#endif

// ---- one dense span: floats [span_first, span_first + span_len) of the tensor `shs` <-> the window ------------------------
// n4 float4s at src4 -> the window, BATCH loads per lane in flight before the first LDS store: with one in flight per wave
// (load, wait, store, next load) the forward's colour kernel ran at the 2 TB/s that 12 waves/CU x 1 KB per memory latency
// allow.  Twelve cover a full degree-3 span (64 rows x 192 B); the backward takes six (twelve cost it a wave of occupancy).
template <bool ROWS48, int BATCH, class T4>
__device__ __forceinline__ void stage_span_vec(T4* __restrict__ src4, int n4, float* lds, int lane)
{
    for (int base = 0; base < n4; base += 64 * BATCH) {
        float4 v[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; k++) {
            const int e4 = base + k * 64 + lane;
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e4 < n4) v[k] = src4[e4];
        }
#pragma unroll
        for (int k = 0; k < BATCH; k++) {
            const int e4 = base + k * 64 + lane;
            if (e4 < n4) {
                const int e = e4 << 2;
                if (ROWS48) {   // 48 % 4 == 0: the four floats are in one row
                    float* d = lds + sh_skew<true>(e);
                    d[0] = v[k].x;
                    d[1] = v[k].y;
                    d[2] = v[k].z;
                    d[3] = v[k].w;
                } else {
                    lds[sh_skew<false>(e)] = v[k].x;
                    lds[sh_skew<false>(e + 1)] = v[k].y;
                    lds[sh_skew<false>(e + 2)] = v[k].z;
                    lds[sh_skew<false>(e + 3)] = v[k].w;
                }
            }
        }
    }
}

// The span -> the window.  A span that starts on a multiple of four floats and is a multiple of four long (always so for
// M = 16) moves as float4s, any other float by float.  rows48 is an argument (wave-uniform), not a template parameter:
// the forward's colour role serves every M from one kernel; the backward passes its ROWS48 and the test folds away.
template <int BATCH, class T>
__device__ __forceinline__ void stage_span(T* shs, long span_first, int span_len, bool rows48, float* lds, int lane)
{
    T* src = shs + span_first;
    if (((span_first | span_len) & 3) == 0) {
        if (rows48)
            stage_span_vec<true, BATCH>(as_float4(src), span_len >> 2, lds, lane);
        else
            stage_span_vec<false, BATCH>(as_float4(src), span_len >> 2, lds, lane);
    } else {
        for (int e = lane; e < span_len; e += 64) lds[rows48 ? sh_skew<true>(e) : sh_skew<false>(e)] = src[e];
    }
}

// the window -> the span (the gradient rows), or zeros when the wave built no rows (`rows` is wave-uniform)
template <bool ROWS48, class T>
__device__ __forceinline__ void unstage_span(T* out, long span_first, int span_len, const float* lds, int lane, bool rows)
{
    T* dst = out + span_first;
    if (((span_first | span_len) & 3) == 0) {
        auto* dst4 = as_float4(dst);
        const int n4 = span_len >> 2;
        if (rows) {
            for (int e4 = lane; e4 < n4; e4 += 64) {
                const int e = e4 << 2;
                if (ROWS48) {
                    const float* q = lds + sh_skew<true>(e);
                    dst4[e4] = make_float4(q[0], q[1], q[2], q[3]);
                } else {
                    dst4[e4] = make_float4(lds[sh_skew<false>(e)], lds[sh_skew<false>(e + 1)], lds[sh_skew<false>(e + 2)],
                                           lds[sh_skew<false>(e + 3)]);
                }
            }
        } else {
            for (int e4 = lane; e4 < n4; e4 += 64) dst4[e4] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else if (rows) {
        for (int e = lane; e < span_len; e += 64) dst[e] = lds[sh_skew<ROWS48>(e)];
    } else {
        for (int e = lane; e < span_len; e += 64) dst[e] = 0.f;
    }
}

// ---- the two spans of split rows <-> the window ------------------------------------------------------------------------------
// one span (len floats at src; 16-byte aligned and len % 4 == 0 when VEC) -> the window, six float4 loads per lane in flight
template <bool ROWS48, bool VEC, class T>
__device__ __forceinline__ void stage_split_span(T* __restrict__ src, int len, int rl, int k0, int M, float* lds, int lane)
{
    if (VEC) {
        constexpr int kBatch = 6;
        const auto* src4 = as_float4(src);
        const int n4 = len >> 2;
        for (int base = 0; base < n4; base += 64 * kBatch) {
            float4 v[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const int e4 = base + k * 64 + lane;
                v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e4 < n4) v[k] = src4[e4];
            }
#pragma unroll
            for (int k = 0; k < kBatch; k++) {
                const int e4 = base + k * 64 + lane;
                if (e4 < n4) {
                    const int f = e4 << 2;
                    lds[sh_split_index<ROWS48>(f, rl, k0, M)] = v[k].x;
                    lds[sh_split_index<ROWS48>(f + 1, rl, k0, M)] = v[k].y;
                    lds[sh_split_index<ROWS48>(f + 2, rl, k0, M)] = v[k].z;
                    lds[sh_split_index<ROWS48>(f + 3, rl, k0, M)] = v[k].w;
                }
            }
        }
    } else {
        for (int f = lane; f < len; f += 64) lds[sh_split_index<ROWS48>(f, rl, k0, M)] = src[f];
    }
}

// the window -> one span, or zeros when the wave built no rows
template <bool ROWS48, bool VEC, class T>
__device__ __forceinline__ void unstage_split_span(T* __restrict__ dst, int len, int rl, int k0, int M, const float* lds, int lane,
                                                   bool rows)
{
    if (VEC) {
        auto* dst4 = as_float4(dst);
        const int n4 = len >> 2;
        if (rows) {
            for (int e4 = lane; e4 < n4; e4 += 64) {
                const int f = e4 << 2;
                dst4[e4] = make_float4(lds[sh_split_index<ROWS48>(f, rl, k0, M)], lds[sh_split_index<ROWS48>(f + 1, rl, k0, M)],
                                       lds[sh_split_index<ROWS48>(f + 2, rl, k0, M)], lds[sh_split_index<ROWS48>(f + 3, rl, k0, M)]);
            }
        } else {
            for (int e4 = lane; e4 < n4; e4 += 64) dst4[e4] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else if (rows) {
        for (int f = lane; f < len; f += 64) dst[f] = lds[sh_split_index<ROWS48>(f, rl, k0, M)];
    } else {
        for (int f = lane; f < len; f += 64) dst[f] = 0.f;
    }
}

// Both spans of the wave's `nrows` rows starting at Gaussian wave_first (a multiple of 64, so both spans start 16-byte
// aligned; full waves have lengths % 4 == 0), into the window ...
template <bool ROWS48, class T>
__device__ __forceinline__ void stage_split_rows(T* dc, T* rest, int wave_first, int nrows, int M, float* lds,
                                                 int lane)
{
    const int rl = 3 * (M - 1);
    T* s_dc = dc + 3L * wave_first;
    T* s_rest = rest + (long)rl * wave_first;
    if ((nrows & 3) == 0) {
        stage_split_span<ROWS48, true>(s_dc, 3 * nrows, 3, 0, M, lds, lane);
        if (M > 1) stage_split_span<ROWS48, true>(s_rest, rl * nrows, rl, 3, M, lds, lane);
    } else {
        stage_split_span<ROWS48, false>(s_dc, 3 * nrows, 3, 0, M, lds, lane);
        if (M > 1) stage_split_span<ROWS48, false>(s_rest, rl * nrows, rl, 3, M, lds, lane);
    }
}

// ... and out of it
template <bool ROWS48, class T>
__device__ __forceinline__ void unstage_split_rows(T* dc, T* rest, int wave_first, int nrows, int M,
                                                   const float* lds, int lane, bool rows)
{
    const int rl = 3 * (M - 1);
    T* d_dc = dc + 3L * wave_first;
    T* d_rest = rest + (long)rl * wave_first;
    if ((nrows & 3) == 0) {
        unstage_split_span<ROWS48, true>(d_dc, 3 * nrows, 3, 0, M, lds, lane, rows);
        if (M > 1) unstage_split_span<ROWS48, true>(d_rest, rl * nrows, rl, 3, M, lds, lane, rows);
    } else {
        unstage_split_span<ROWS48, false>(d_dc, 3 * nrows, 3, 0, M, lds, lane, rows);
        if (M > 1) unstage_split_span<ROWS48, false>(d_rest, rl * nrows, rl, 3, M, lds, lane, rows);
    }
}

}  // namespace r3

#endif
