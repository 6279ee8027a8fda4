// mip.hip -- the anti-aliasing unit of include/r3dgs_mip.h: the per-view 2D opacity compensation and the 3D smoothing filter,
// both as maps from raw parameters to raw parameters in front of the unchanged rasterizer.  Per-Gaussian arithmetic: mip_math.h.
//
// wave64, 256-thread workgroups, no float atomics, no host wait, no allocation; every kernel is P-sized and HBM-bound.
//   opacity            one lane per Gaussian; the view matrix is staged in LDS once per workgroup (16 floats, read as LDS
//                      broadcasts).  44 B read (40 with a precomputed covariance), 4 B written (+ 4 with rho).
//   opacity backward   one lane per Gaussian, the forward recomputed from the inputs (nothing is kept between the two):
//                      48 B read, up to 44 B written.  The chain from d rho to the mean, scale and quaternion runs in double.
//   filter3d  scan     one lane per Gaussian loops over the V cameras; the camera table arrives through LDS in chunks of
//                      kCamChunk rows (80 B each), uniform across the workgroup.  Writes the Gaussian's filter value, or -1 if
//                      no camera sees it, and per workgroup the maximum of the depths' bit patterns (positive floats: the
//                      integer order is the float order).  12 B read, 4 B written.
//             finish   ONE workgroup: the global maximum of the per-workgroup words, the largest focal length, and the fill of
//                      the rows marked -1.  4 B read per Gaussian, 4 B written per filled row.
//   filtered           one lane per Gaussian: 20 B read, 16 B written; backward 36 B read, 16 B written.  f == 0 copies.
#include "../../include/r3dgs_mip.h"

#include "common.h"
#include "mip_math.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kFinishBlock = 1024;
constexpr int kCamChunk = 64;   // camera rows staged per round: 5 KB of LDS
constexpr long long kMaxP = 1LL << 30;
static_assert(r3::kMipCamFloats == R3DGS_MIP_CAMERA_FLOATS, "the camera row of the header");

inline long long blocks_of(long long P) { return (P + kBlock - 1) / kBlock; }

struct __attribute__((packed, aligned(4))) Row3 {
    float v[3];
};
struct __attribute__((packed, aligned(4))) Row6 {
    float v[6];
};

struct OpacityArgs {
    int P, raw;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* cov6;
    const float* opacities;
    const float* view;
    float tan_fovx, tan_fovy;
    int W, H;
    float scale_modifier;
};

// The workgroup's view, through LDS: every thread of the workgroup calls it.
// (The helpers take the block's fields by value: a reference to the by-value kernel argument would spill it to scratch.)
__device__ __forceinline__ r3::MipView stage_view(const float* view, float tan_fovx, float tan_fovy, int W, int H,
                                                  float scale_modifier, float* s_view)
{
    if (threadIdx.x < 16) s_view[threadIdx.x] = view[threadIdx.x];
    __syncthreads();
    return r3::mip_make_view(s_view, tan_fovx, tan_fovy, W, H, scale_modifier);
}

// One Gaussian's inputs, every load issued before anything waits on one of them.  raw: scale / q are activated here and
// `n` is the quaternion's norm (for the backward); s_raw / q_raw keep what was loaded.
struct Lane {
    float m[3], scale[3], q[4], cov6[6], o, n;
};
// COV: the covariance is precomputed (a template parameter, not a pointer test at run time: a pointer chosen at run time
// keeps the lane's arrays in scratch)
template <bool RAW, bool COV>
__device__ __forceinline__ Lane load_lane(const float* means3D, const float* scales, const float* rotations, const float* cov6,
                                          const float* opacities, size_t i, float* q_raw)
{
    Lane L;
    const Row3 m = reinterpret_cast<const Row3*>(means3D)[i];
    L.o = opacities[i];
    L.n = 1.f;
    if (COV) {
        const Row6 c = reinterpret_cast<const Row6*>(cov6)[i];
#pragma unroll
        for (int k = 0; k < 6; k++) L.cov6[k] = c.v[k];
#pragma unroll
        for (int k = 0; k < 3; k++) L.scale[k] = 1.f;
        L.q[0] = 1.f;
        L.q[1] = L.q[2] = L.q[3] = 0.f;
    } else {
        const float4 q4 = reinterpret_cast<const float4*>(rotations)[i];
        const Row3 s = reinterpret_cast<const Row3*>(scales)[i];
        const float q[4] = {q4.x, q4.y, q4.z, q4.w};
        if (RAW) {
#pragma unroll
            for (int k = 0; k < 3; k++) L.scale[k] = r3::scale_act(s.v[k]);
            L.n = r3::quat_act(q, L.q);
#pragma unroll
            for (int k = 0; k < 4; k++) q_raw[k] = q[k];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) L.scale[k] = s.v[k];
#pragma unroll
            for (int k = 0; k < 4; k++) L.q[k] = q[k];
        }
#pragma unroll
        for (int k = 0; k < 6; k++) L.cov6[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) L.m[k] = m.v[k];
    return L;
}

template <bool RAW, bool COV>
__global__ __launch_bounds__(kBlock) void opacity_kernel(const OpacityArgs a, float* __restrict__ raw_eff, float* __restrict__ rho)
{
    __shared__ float s_view[16];
    const r3::MipView v = stage_view(a.view, a.tan_fovx, a.tan_fovy, a.W, a.H, a.scale_modifier, s_view);
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)a.P) return;
    float q_raw[4];
    const Lane L = load_lane<RAW, COV>(a.means3D, a.scales, a.rotations, a.cov6, a.opacities, i, q_raw);
    float r;
    raw_eff[i] = r3::mip_opacity_one(v, L.m, L.scale, L.q, COV ? L.cov6 : nullptr, L.o, &r);
    if (rho) rho[i] = r;
}

struct OpacityGrads {
    float* d_o;
    float* d_means;
    float* d_scales;
    float* d_rot;
    float* d_cov;
};

template <bool RAW, bool COV>
__global__ __launch_bounds__(kBlock) void opacity_bwd_kernel(const OpacityArgs a, const float* __restrict__ g, const OpacityGrads out)
{
    __shared__ float s_view[16];
    const r3::MipView v = stage_view(a.view, a.tan_fovx, a.tan_fovy, a.W, a.H, a.scale_modifier, s_view);
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)a.P) return;
    float q_raw[4] = {0.f, 0.f, 0.f, 0.f};
    const Lane L = load_lane<RAW, COV>(a.means3D, a.scales, a.rotations, a.cov6, a.opacities, i, q_raw);
    const float gi = g[i];
    float d_o, dmean[3], dscale[3], dq[4], dcov[6];
    r3::mip_opacity_bwd_one(v, L.m, L.scale, L.q, COV ? L.cov6 : nullptr, L.o, gi, &d_o, dmean, dscale, dq, dcov);
    if (RAW) {   // through the activations, as the raw-parameter backward does (param_math.h)
        float dq_raw[4];
        r3::quat_act_bwd(L.q, L.n, dq, dq_raw);
#pragma unroll
        for (int k = 0; k < 4; k++) dq[k] = dq_raw[k];
#pragma unroll
        for (int k = 0; k < 3; k++) dscale[k] = r3::scale_act_bwd(dscale[k], L.scale[k]);
    }
    if (out.d_o) out.d_o[i] = d_o;
    if (out.d_means) {
        Row3 r;
#pragma unroll
        for (int k = 0; k < 3; k++) r.v[k] = dmean[k];
        reinterpret_cast<Row3*>(out.d_means)[i] = r;
    }
    if (out.d_scales) {
        Row3 r;
#pragma unroll
        for (int k = 0; k < 3; k++) r.v[k] = dscale[k];
        reinterpret_cast<Row3*>(out.d_scales)[i] = r;
    }
    if (out.d_rot) {
        Row3 lo;   // [P,4] rows need not be 16-byte aligned on the way out: a 12-byte and a 4-byte store
        lo.v[0] = dq[0];
        lo.v[1] = dq[1];
        lo.v[2] = dq[2];
        *reinterpret_cast<Row3*>(out.d_rot + 4 * i) = lo;
        out.d_rot[4 * i + 3] = dq[3];
    }
    if (out.d_cov) {
        Row6 r;
#pragma unroll
        for (int k = 0; k < 6; k++) r.v[k] = dcov[k];
        reinterpret_cast<Row6*>(out.d_cov)[i] = r;
    }
}

// ---- 3D filter -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, off);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(kBlock) void filter_scan_kernel(int P, int V, const float* __restrict__ means3D,
                                                             const float* __restrict__ cameras, float* __restrict__ filter,
                                                             uint32_t* __restrict__ block_max)
{
    __shared__ float s_cam[kCamChunk * r3::kMipCamFloats];
    __shared__ uint32_t s_max[kWaves];
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kBlock + tid;
    const bool in = i < (size_t)P;
    float m[3] = {0.f, 0.f, 0.f};
    if (in) {
        const Row3 r = reinterpret_cast<const Row3*>(means3D)[i];
        m[0] = r.v[0];
        m[1] = r.v[1];
        m[2] = r.v[2];
    }
    float d = 0.f, focal_max = 0.f;   // d: 0 = no valid camera yet (a valid depth is > 0.2)
    for (int v0 = 0; v0 < V; v0 += kCamChunk) {
        const int n = V - v0 < kCamChunk ? V - v0 : kCamChunk;
        __syncthreads();   // the previous round's readers are done
        for (int k = tid; k < n * r3::kMipCamFloats; k += kBlock) s_cam[k] = cameras[(size_t)v0 * r3::kMipCamFloats + k];
        __syncthreads();
        for (int c = 0; c < n; c++) {
            const float* cam = s_cam + c * r3::kMipCamFloats;
            focal_max = r3::fmax_(focal_max, cam[16]);
            const float z = in ? r3::mip_filter_valid(cam, m) : 0.f;
            if (z > 0.f) d = d > 0.f ? r3::fmin_(d, z) : z;
        }
    }
    if (in) filter[i] = d > 0.f ? r3::mip_filter_value(d, focal_max) : -1.f;
    const uint32_t w = wave_max_u32(__float_as_uint(d));
    if ((tid & 63) == 0) s_max[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        uint32_t x = s_max[0];
#pragma unroll
        for (int k = 1; k < kWaves; k++) x = s_max[k] > x ? s_max[k] : x;
        block_max[blockIdx.x] = x;
    }
}

__global__ __launch_bounds__(kFinishBlock) void filter_finish_kernel(int P, int V, long long nb, const float* __restrict__ cameras,
                                                                     const uint32_t* __restrict__ block_max, float* __restrict__ filter)
{
    __shared__ uint32_t s_d[kFinishBlock / 64], s_f[kFinishBlock / 64];
    const int tid = threadIdx.x;
    uint32_t dmax = 0u, fmax = 0u;   // bit patterns of non-negative floats
    for (long long b = tid; b < nb; b += kFinishBlock) dmax = block_max[b] > dmax ? block_max[b] : dmax;
    for (int v = tid; v < V; v += kFinishBlock) {
        const float f = r3::fmax_(0.f, cameras[(size_t)v * r3::kMipCamFloats + 16]);
        const uint32_t u = __float_as_uint(f);
        fmax = u > fmax ? u : fmax;
    }
    dmax = wave_max_u32(dmax);
    fmax = wave_max_u32(fmax);
    if ((tid & 63) == 0) {
        s_d[tid >> 6] = dmax;
        s_f[tid >> 6] = fmax;
    }
    __syncthreads();
    dmax = fmax = 0u;
#pragma unroll
    for (int k = 0; k < kFinishBlock / 64; k++) {
        dmax = s_d[k] > dmax ? s_d[k] : dmax;
        fmax = s_f[k] > fmax ? s_f[k] : fmax;
    }
    const float d = __uint_as_float(dmax);
    const float fill = d > 0.f ? r3::mip_filter_value(d, __uint_as_float(fmax)) : 0.f;
    for (size_t i = (size_t)tid; i < (size_t)P; i += kFinishBlock)
        if (filter[i] < 0.f) filter[i] = fill;
}

__global__ __launch_bounds__(kBlock) void filtered_kernel(int P, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                          const float* __restrict__ filter, float* __restrict__ scaling_eff,
                                                          float* __restrict__ opacity_eff)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P) return;
    const Row3 ls = reinterpret_cast<const Row3*>(scaling)[i];
    const float o = opacity[i], f = filter[i];
    Row3 out;
    float raw;
    r3::mip_filtered_one(ls.v, o, f, out.v, &raw);
    reinterpret_cast<Row3*>(scaling_eff)[i] = out;
    opacity_eff[i] = raw;
}

__global__ __launch_bounds__(kBlock) void filtered_bwd_kernel(int P, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                              const float* __restrict__ filter, const float* __restrict__ g_scaling,
                                                              const float* __restrict__ g_opacity, float* __restrict__ d_scaling,
                                                              float* __restrict__ d_opacity)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P) return;
    const Row3 ls = reinterpret_cast<const Row3*>(scaling)[i];
    const float o = opacity[i], f = filter[i];
    Row3 g{{0.f, 0.f, 0.f}};
    if (g_scaling) g = reinterpret_cast<const Row3*>(g_scaling)[i];
    const float go = g_opacity ? g_opacity[i] : 0.f;
    Row3 out;
    float d_o;
    r3::mip_filtered_bwd_one(ls.v, o, f, g.v, go, out.v, &d_o);
    if (d_scaling) reinterpret_cast<Row3*>(d_scaling)[i] = out;
    if (d_opacity) d_opacity[i] = d_o;
}

OpacityArgs checked_opacity_args(const char* what, int P, const float* means3D, const float* scales, const float* rotations,
                                 const float* cov6, const float* opacities, int raw, const float* view, float tan_fovx,
                                 float tan_fovy, int W, int H, float scale_modifier)
{
    const std::string w(what);
    if (P > kMaxP) throw r3::Error(w + ": P exceeds 2^30");
    if (!means3D || !opacities || !view) throw r3::Error(w + ": means3D, opacities or viewmatrix is NULL");
    if (cov6) {
        if (raw) throw r3::Error(w + ": raw parameters and cov3D_precomp exclude each other");
    } else {
        if (!scales || !rotations) throw r3::Error(w + ": neither cov3D_precomp nor a scale / rotation pair");
        if ((uintptr_t)rotations % 16) throw r3::Error(w + ": rotations must be 16-byte aligned");
    }
    if ((uintptr_t)means3D % 4 || (uintptr_t)opacities % 4 || (uintptr_t)view % 4 || (uintptr_t)scales % 4 || (uintptr_t)cov6 % 4)
        throw r3::Error(w + ": a tensor is not 4-byte aligned");
    if (W <= 0 || H <= 0 || !(tan_fovx > 0.f) || !(tan_fovy > 0.f)) throw r3::Error(w + ": W, H, tan_fovx and tan_fovy must be positive");
    OpacityArgs a;
    a.P = P;
    a.raw = raw ? 1 : 0;
    a.means3D = means3D;
    a.scales = scales;
    a.rotations = rotations;
    a.cov6 = cov6;
    a.opacities = opacities;
    a.view = view;
    a.tan_fovx = tan_fovx;
    a.tan_fovy = tan_fovy;
    a.W = W;
    a.H = H;
    a.scale_modifier = scale_modifier;
    return a;
}

}  // namespace

extern "C" {

int r3dgs_mip_opacity(int P, const float* means3D, const float* scales, const float* rotations, const float* cov3D_precomp,
                      const float* opacities, int raw, const float* viewmatrix, float tan_fovx, float tan_fovy, int W, int H,
                      float scale_modifier, float* raw_eff, float* rho, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        const OpacityArgs a = checked_opacity_args("mip_opacity", P, means3D, scales, rotations, cov3D_precomp, opacities, raw,
                                                   viewmatrix, tan_fovx, tan_fovy, W, H, scale_modifier);
        if (!raw_eff || (uintptr_t)raw_eff % 4 || (uintptr_t)rho % 4) throw r3::Error("mip_opacity: raw_eff is NULL, or an output is not 4-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (a.cov6)
            opacity_kernel<false, true><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, raw_eff, rho);
        else if (a.raw)
            opacity_kernel<true, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, raw_eff, rho);
        else
            opacity_kernel<false, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, raw_eff, rho);
        r3::check_launch("mip opacity", s, false);
        return 0;
    });
}

int r3dgs_mip_opacity_backward(int P, const float* means3D, const float* scales, const float* rotations,
                               const float* cov3D_precomp, const float* opacities, int raw, const float* viewmatrix,
                               float tan_fovx, float tan_fovy, int W, int H, float scale_modifier, const float* dL_draw_eff,
                               float* dL_dopacities, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                               float* dL_dcov3D, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        const OpacityArgs a = checked_opacity_args("mip_opacity_backward", P, means3D, scales, rotations, cov3D_precomp, opacities,
                                                   raw, viewmatrix, tan_fovx, tan_fovy, W, H, scale_modifier);
        if (!dL_draw_eff || (uintptr_t)dL_draw_eff % 4) throw r3::Error("mip_opacity_backward: dL_draw_eff is NULL or not 4-byte aligned");
        const OpacityGrads out{dL_dopacities, dL_dmeans3D, dL_dscales, dL_drotations, dL_dcov3D};
        if ((uintptr_t)out.d_o % 4 || (uintptr_t)out.d_means % 4 || (uintptr_t)out.d_scales % 4 || (uintptr_t)out.d_rot % 4 ||
            (uintptr_t)out.d_cov % 4)
            throw r3::Error("mip_opacity_backward: an output is not 4-byte aligned");
        if (!out.d_o && !out.d_means && !out.d_scales && !out.d_rot && !out.d_cov) return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (a.cov6)
            opacity_bwd_kernel<false, true><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, dL_draw_eff, out);
        else if (a.raw)
            opacity_bwd_kernel<true, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, dL_draw_eff, out);
        else
            opacity_bwd_kernel<false, false><<<(unsigned)blocks_of(P), kBlock, 0, s>>>(a, dL_draw_eff, out);
        r3::check_launch("mip opacity backward", s, false);
        return 0;
    });
}

size_t r3dgs_mip_filter3d_workspace_bytes(int P, int V)
{
    if (P <= 0 || P > kMaxP || V < 0) return 0;
    return (((size_t)blocks_of(P) * sizeof(uint32_t)) + 15) & ~(size_t)15;
}

int r3dgs_mip_filter3d(int P, int V, const float* means3D, const float* cameras, float* filter, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (P > kMaxP) throw r3::Error("mip_filter3d: P exceeds 2^30");
        if (V < 0 || V > (1 << 24)) throw r3::Error("mip_filter3d: V out of range");
        if (!means3D || !filter || (V > 0 && !cameras)) throw r3::Error("mip_filter3d: means3D, cameras or filter is NULL");
        if ((uintptr_t)means3D % 4 || (uintptr_t)cameras % 4 || (uintptr_t)filter % 4) throw r3::Error("mip_filter3d: a tensor is not 4-byte aligned");
        if (!workspace || (uintptr_t)workspace % 16) throw r3::Error("mip_filter3d: workspace is NULL or not 16-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const long long nb = blocks_of(P);
        uint32_t* block_max = reinterpret_cast<uint32_t*>(workspace);
        filter_scan_kernel<<<(unsigned)nb, kBlock, 0, s>>>(P, V, means3D, cameras, filter, block_max);
        r3::check_launch("mip filter3d scan", s, false);
        filter_finish_kernel<<<1, kFinishBlock, 0, s>>>(P, V, nb, cameras, block_max, filter);
        r3::check_launch("mip filter3d finish", s, false);
        return 0;
    });
}

int r3dgs_mip_filtered(int P, const float* scaling_raw, const float* opacity_raw, const float* filter, float* scaling_eff,
                       float* opacity_eff, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (P > kMaxP) throw r3::Error("mip_filtered: P exceeds 2^30");
        if (!scaling_raw || !opacity_raw || !filter || !scaling_eff || !opacity_eff) throw r3::Error("mip_filtered: a tensor is NULL");
        if ((uintptr_t)scaling_raw % 4 || (uintptr_t)opacity_raw % 4 || (uintptr_t)filter % 4 || (uintptr_t)scaling_eff % 4 ||
            (uintptr_t)opacity_eff % 4)
            throw r3::Error("mip_filtered: a tensor is not 4-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        filtered_kernel<<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, scaling_raw, opacity_raw, filter, scaling_eff, opacity_eff);
        r3::check_launch("mip filtered", s, false);
        return 0;
    });
}

int r3dgs_mip_filtered_backward(int P, const float* scaling_raw, const float* opacity_raw, const float* filter,
                                const float* dL_dscaling_eff, const float* dL_dopacity_eff, float* dL_dscaling_raw,
                                float* dL_dopacity_raw, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (P > kMaxP) throw r3::Error("mip_filtered_backward: P exceeds 2^30");
        if (!scaling_raw || !opacity_raw || !filter) throw r3::Error("mip_filtered_backward: a tensor is NULL");
        if ((uintptr_t)scaling_raw % 4 || (uintptr_t)opacity_raw % 4 || (uintptr_t)filter % 4 || (uintptr_t)dL_dscaling_eff % 4 ||
            (uintptr_t)dL_dopacity_eff % 4 || (uintptr_t)dL_dscaling_raw % 4 || (uintptr_t)dL_dopacity_raw % 4)
            throw r3::Error("mip_filtered_backward: a tensor is not 4-byte aligned");
        if (!dL_dscaling_raw && !dL_dopacity_raw) return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        filtered_bwd_kernel<<<(unsigned)blocks_of(P), kBlock, 0, s>>>(P, scaling_raw, opacity_raw, filter, dL_dscaling_eff,
                                                                      dL_dopacity_eff, dL_dscaling_raw, dL_dopacity_raw);
        r3::check_launch("mip filtered backward", s, false);
        return 0;
    });
}

}  // extern "C"
