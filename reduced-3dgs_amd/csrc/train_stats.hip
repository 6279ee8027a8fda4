// train_stats.hip -- the per-iteration training statistics of include/r3dgs_trainstats.h: what the reference's loop computes
// around loss.backward() with boolean-mask indexing (train.py:105-106, :113, :134, scene/gaussian_model.py:693-695), as
// three calls that never wait on the host.  Per-element arithmetic: stats_math.h.
//
// visible_means: one 256-thread workgroup per 256 Gaussians, two phases.
//   * per Gaussian (one lane each): radii -> visibility byte, sigmoid(opacity) of the visible ones into a double;
//   * features_rest (the only real traffic: 12 (M - 1) bytes per Gaussian, 180 at M = 16): the rows of a wave's 64 Gaussians
//     are one contiguous run of 64 * 3 (M - 1) floats that starts 16-byte aligned whenever the tensor does, so the wave walks
//     it in 16-byte words, lane l taking word l, l + 64, ... (a wave instruction covers 1 KB contiguous) and a lane issues the
//     load only if its word overlaps the row of a Gaussian whose bit is set in the wave's visibility ballot.  One lane per
//     row would be 64 lanes striding 180 B.  kUnroll words per lane are requested before any is summed.
//   A tensor that is not 16-byte aligned (a view) takes the same walk with 4-byte words.
// Sums are doubles: per lane in index order, per wave by a fixed shuffle tree, per workgroup in wave order.  The
// workgroup's three partials go to the caller's workspace, and a second one-workgroup launch adds them in a fixed order
// (thread t takes partials t, t + 256, ...; the same tree) and divides.  No atomics: run-to-run bit-identical.
// Why double: the terms are fp32 values, so each partial sum is exact to 2^-53 relative and the result is the correctly
// rounded mean up to the final fp32 rounding, for any P, M and summation shape; an fp32 tree over 22 M terms (500 k x 45)
// would carry ~1e-6 that depends on how the work was cut.
#include "../../include/r3dgs_trainstats.h"

#include "common.h"
#include "stats_math.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kUnroll = 4;   // words of features_rest a lane has in flight: 4 x 16 B

struct Partials {   // per workgroup of visible_means_kernel, in the caller's workspace
    double* alpha;  // [nb] sum of sigmoid(opacity) over the workgroup's visible Gaussians
    double* sh;     // [nb] sum of |features_rest| over their rows
    int* count;     // [nb] visible Gaussians
};
inline long long stats_blocks(long long P) { return (P + kBlock - 1) / kBlock; }
inline Partials carve_partials(char* ws, long long nb)
{
    Partials p;
    p.alpha = reinterpret_cast<double*>(ws);
    p.sh = p.alpha + nb;
    p.count = reinterpret_cast<int*>(p.sh + nb);
    return p;
}

// lane 0 receives ((v0 + v32) + (v16 + v48)) + ...: a fixed tree
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// VEC floats per word: 4 (features_rest 16-byte aligned) or 1.  R = 3 (M - 1) floats per row, 0: no rows.
template <int VEC>
__global__ __launch_bounds__(kBlock) void visible_means_kernel(int P, int R, const int* __restrict__ radii,
                                                               const float* __restrict__ opacity,
                                                               const float* __restrict__ rest,
                                                               uint8_t* __restrict__ visibility, Partials out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i = (long long)blockIdx.x * kBlock + tid;
    bool vis = false;
    double alpha = 0.0;
    if (i < P) {
        vis = radii[i] > 0;
        visibility[i] = vis ? 1 : 0;
        if (opacity && vis) alpha = (double)r3::stats_sigmoid(opacity[i]);
    }
    const unsigned long long vmask = __ballot(vis);

    double sh = 0.0;
    if (R > 0 && vmask) {   // wave-uniform
        const long long g0 = (long long)blockIdx.x * kBlock + wave * 64;   // the wave's first Gaussian (< P: one is visible)
        const float* __restrict__ base = rest + g0 * R;
        const long long left = (long long)P - g0;
        const uint32_t avail = (uint32_t)(left < 64 ? left : 64) * (uint32_t)R;   // floats of the wave's rows that exist
        const uint32_t words = (avail + VEC - 1) / VEC;
        for (uint32_t w0 = 0; w0 < words; w0 += 64 * kUnroll) {
            float v[kUnroll][VEC];
            uint32_t need[kUnroll];   // bit k: element k of the word lies in a visible Gaussian's row
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const uint32_t e0 = (w0 + u * 64 + lane) * VEC;
                const uint32_t row0 = e0 / (uint32_t)R, rem = e0 - row0 * (uint32_t)R;
                need[u] = 0;
#pragma unroll
                for (int k = 0; k < VEC; k++) {
                    v[u][k] = 0.f;
                    // R >= 3 and k <= 3: a word spans at most two rows
                    const uint32_t row = row0 + (rem + k >= (uint32_t)R ? 1u : 0u);
                    if (e0 + k < avail && ((vmask >> row) & 1ull)) need[u] |= 1u << k;
                }
                if (need[u]) {
                    bool whole = false;
                    if constexpr (VEC == 4) {
                        if (e0 + 3 < avail) {   // the whole word exists (it may overlap a culled Gaussian's row)
                            const float4 q = *reinterpret_cast<const float4*>(base + e0);
                            v[u][0] = q.x;
                            v[u][1] = q.y;
                            v[u][2] = q.z;
                            v[u][3] = q.w;
                            whole = true;
                        }
                    }
                    if (!whole) {
#pragma unroll
                        for (int k = 0; k < VEC; k++)
                            if (need[u] >> k & 1u) v[u][k] = base[e0 + k];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++)
#pragma unroll
                for (int k = 0; k < VEC; k++)
                    if (need[u] >> k & 1u) sh += (double)fabsf(v[u][k]);
        }
    }

    __shared__ double s_alpha[kWaves], s_sh[kWaves];
    __shared__ int s_count[kWaves];
    alpha = wave_sum(alpha);
    sh = wave_sum(sh);
    if (lane == 0) {
        s_alpha[wave] = alpha;
        s_sh[wave] = sh;
        s_count[wave] = __popcll(vmask);
    }
    __syncthreads();
    if (tid == 0) {
        double a = s_alpha[0], s = s_sh[0];
        int c = s_count[0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) {
            a += s_alpha[w];
            s += s_sh[w];
            c += s_count[w];
        }
        out.alpha[blockIdx.x] = a;
        out.sh[blockIdx.x] = s;
        out.count[blockIdx.x] = c;
    }
}

// One workgroup: the nb partials in a fixed order, then the two divisions.  0 / 0 = NaN is torch's mean of nothing.
__global__ __launch_bounds__(kBlock) void visible_means_finish_kernel(long long nb, int R, Partials in,
                                                                      int* __restrict__ n_visible,
                                                                      float* __restrict__ alpha_mean,
                                                                      float* __restrict__ sh_abs_mean)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double alpha = 0.0, sh = 0.0;
    long long count = 0;
    for (long long b = tid; b < nb; b += kBlock) {
        alpha += in.alpha[b];
        sh += in.sh[b];
        count += in.count[b];
    }
    __shared__ double s_alpha[kWaves], s_sh[kWaves];
    __shared__ long long s_count[kWaves];
    alpha = wave_sum(alpha);
    sh = wave_sum(sh);
    count = wave_sum(count);
    if (lane == 0) {
        s_alpha[wave] = alpha;
        s_sh[wave] = sh;
        s_count[wave] = count;
    }
    __syncthreads();
    if (tid != 0) return;
    double a = s_alpha[0], s = s_sh[0];
    long long c = s_count[0];
#pragma unroll
    for (int w = 1; w < kWaves; w++) {
        a += s_alpha[w];
        s += s_sh[w];
        c += s_count[w];
    }
    *n_visible = (int)c;
    const double n = (double)c;
    if (alpha_mean) *alpha_mean = (float)(a / n);
    if (sh_abs_mean) *sh_abs_mean = R > 0 ? (float)(s / (n * (double)R)) : __builtin_nanf("");
}

__global__ __launch_bounds__(kBlock) void alpha_regul_backward_kernel(int P, const int* __restrict__ radii,
                                                                      const float* __restrict__ opacity,
                                                                      const float* __restrict__ upstream,
                                                                      const int* __restrict__ n_visible,
                                                                      float* __restrict__ dL_dopacity)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= P || radii[i] <= 0) return;
    const int n = *n_visible;   // wave-uniform addresses: scalar loads
    if (n <= 0) return;
    const float scale = *upstream / (float)n;
    dL_dopacity[i] = dL_dopacity[i] + r3::alpha_regul_term(opacity[i], scale);
}

// gaussian_model.py:693-695 adds the norm of every row of viewspace.grad, not only the visible ones: the backward writes
// all-zero rows for culled Gaussians (radii == 0), so adding 0 for them -- without reading the row -- is the same update.
__global__ __launch_bounds__(kBlock) void densification_stats_kernel(int P, const float* __restrict__ vg,
                                                                     const int* __restrict__ radii,
                                                                     float* __restrict__ grad_accum,
                                                                     float* __restrict__ denom,
                                                                     float* __restrict__ max_radii)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    float gx = 0.f, gy = 0.f;
    if (r > 0) {
        gx = vg[3 * i];
        gy = vg[3 * i + 1];
    }
    float a = grad_accum[i], d = denom[i], m = max_radii[i];
    r3::densify_update(r, gx, gy, a, d, m);
    grad_accum[i] = a;
    denom[i] = d;
    max_radii[i] = m;
}

}  // namespace

extern "C" {

size_t r3dgs_train_stats_workspace_bytes(int P)
{
    if (P <= 0) return 0;
    const size_t nb = (size_t)stats_blocks(P);
    return (nb * (2 * sizeof(double) + sizeof(int)) + r3::kAlign - 1) & ~(r3::kAlign - 1);
}

int r3dgs_visible_means(int P, int M, const int* radii, const float* opacity, const float* features_rest,
                        uint8_t* visibility, int* n_visible, float* alpha_mean, float* sh_abs_mean, char* workspace,
                        void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (M < 1) throw r3::Error("visible_means: M must be >= 1 (it counts the DC coefficient)");
        if (!radii || !visibility || !n_visible || !workspace) throw r3::Error("visible_means: a required pointer is NULL");
        if (alpha_mean && !opacity) throw r3::Error("visible_means: alpha_mean wanted but opacity is NULL");
        const bool rows = sh_abs_mean && M > 1;   // M == 1: sh_abs_mean is the mean of nothing, no row exists
        if (rows && !features_rest) throw r3::Error("visible_means: sh_abs_mean wanted but features_rest is NULL");
        if ((uintptr_t)workspace % 8) throw r3::Error("visible_means: workspace must be 8-byte aligned");
        if (rows && (uintptr_t)features_rest % 4) throw r3::Error("visible_means: features_rest is not 4-byte aligned");
        if (M > (1 << 20)) throw r3::Error("visible_means: M is too large");
        const int R = rows ? 3 * (M - 1) : 0;
        const float* op = alpha_mean ? opacity : nullptr;
        const float* rest = rows ? features_rest : nullptr;
        hipStream_t s = static_cast<hipStream_t>(stream);
        const long long nb = stats_blocks(P);
        const Partials parts = carve_partials(workspace, nb);
        if (rows && (uintptr_t)rest % 16 == 0)
            visible_means_kernel<4><<<(unsigned)nb, kBlock, 0, s>>>(P, R, radii, op, rest, visibility, parts);
        else
            visible_means_kernel<1><<<(unsigned)nb, kBlock, 0, s>>>(P, R, radii, op, rest, visibility, parts);
        r3::check_launch("visible means", s, false);
        visible_means_finish_kernel<<<1, kBlock, 0, s>>>(nb, R, parts, n_visible, alpha_mean, sh_abs_mean);
        r3::check_launch("visible means (finish)", s, false);
        return 0;
    });
}

int r3dgs_alpha_regul_backward(int P, const int* radii, const float* opacity, const float* upstream, const int* n_visible,
                               float* dL_dopacity, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (!radii || !opacity || !upstream || !n_visible || !dL_dopacity)
            throw r3::Error("alpha_regul_backward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        alpha_regul_backward_kernel<<<(unsigned)stats_blocks(P), kBlock, 0, s>>>(P, radii, opacity, upstream, n_visible,
                                                                                dL_dopacity);
        r3::check_launch("alpha regul backward", s, false);
        return 0;
    });
}

int r3dgs_densification_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum, float* denom,
                              float* max_radii2D, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (!viewspace_grad || !radii || !xyz_gradient_accum || !denom || !max_radii2D)
            throw r3::Error("densification_stats: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        densification_stats_kernel<<<(unsigned)stats_blocks(P), kBlock, 0, s>>>(P, viewspace_grad, radii, xyz_gradient_accum,
                                                                               denom, max_radii2D);
        r3::check_launch("densification stats", s, false);
        return 0;
    });
}

}  // extern "C"
