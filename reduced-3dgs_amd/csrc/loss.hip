// loss.hip -- the fused L1 + D-SSIM training loss (include/r3dgs_loss.h), plain and behind a per-image exposure and a pixel
// mask (r3dgs_exposure_loss_*), forward and backward.
//
// What the reference does (utils/loss_utils.py:17-66, train.py:109-115): five 11x11 depthwise F.conv2d calls with zero
// padding 5 (mu_x, mu_y, E[x^2], E[y^2], E[xy]), about fifteen elementwise ops and autograd's backward of all of them --
// ~15 full-size intermediate maps forward and twice as many backward.  How it is issued here, on the tile filter of
// ssim_tile.h (one workgroup per 64 x 16 output tile of one (image, channel) plane), each step written once:
//   * fwd_tile, the forward of both losses: a pair (x, y) is staged, its five moments filtered, and per pixel loss_math.h
//     gives S and its three partials.  The workgroup writes its sums of S and |x - y| to its own workspace slot; in training
//     mode it also writes the three partial maps (12 B per element).  The two kernels differ in the pair they stage:
//     ssim_fwd_kernel the images themselves (and it may write the S map), exposure_fwd_kernel x'' = m (x E[:, :3] + E[:, 3])
//     and y' = m y or y (exposure_math.h).
//   * loss_reduce_kernel, the reduction of both and of the flat L1 (l1_fwd_kernel): one workgroup adds the slots of each image
//     in a fixed order (ssim_tile.h slot_sums) and writes the means, the per-image means and the combined loss.
//   * bwd_channel, the backward step of one plane: the three partial maps are staged, each scaled by the upstream gradient of
//     S at its pixel; the transpose of a zero-padded convolution with a symmetric window is the same filter over in-image
//     positions, so the gradient with respect to the staged x is
//     g = F[gS dS/dmu_x] + 2x F[gS dS/dE_xx] + y F[gS dS/dE_xy] + g_l1 sign(x - y) / n.
//     plane_bwd_tile wraps it for one workgroup per (plane, tile): ssim_bwd_kernel is its instantiation with the entry point's
//     three modes of the upstream gradient and dx = g; masked_bwd_kernel (no exposure, any C) the one with a uniform upstream
//     gradient and the mask on x, y and dx.  exposure_bwd_kernel (one workgroup per (image, tile), C = 3) runs the step once
//     per channel on the recomputed x'' and y' and carries g on to x and to E.
// What differs between the instantiations is chosen at compile time: the plain kernels carry no argument, branch or register
// for the exposed ones.  No atomics anywhere: every sum has a fixed order (ssim_tile.h), so values and gradients are identical
// run to run.
#include "../../include/r3dgs_loss.h"

#include "common.h"
#include "exposure_math.h"
#include "loss_math.h"
#include "ssim_tile.h"

using namespace r3;

namespace {

constexpr int kL1Chunk = 4 * kBlock;        // elements per workgroup of the flat L1 kernel

struct FwdArgs {
    Plane p;
    int nblocks;
    const float* x;
    const float* y;
    float* ssim_map;   // may be NULL
    float* partials;   // [3][n] or NULL
    float* slots;      // [2][nblocks]: sum S, sum |x - y|
    long long n;
    Window win;
};

// The tile forward of the plane at `base`: stage(gy, gx, v) gives the pair (x, y) the loss is taken of at an in-image pixel.
// kMap: whether this instantiation may be asked for the S map.
template <bool kMap, class Stage>
__device__ __forceinline__ void fwd_tile(const FwdArgs& a, const Tile& tl, size_t base, Stage stage)
{
    __shared__ float sxy[2][kInH][kInW];
    __shared__ float sh[5][kInH][kTW];
    __shared__ float red[2][kBlock / 64];
    const int W = a.p.W;
    stage_tiles(a.p, tl, sxy, stage);
    float acc[kRows][5];
    filter_tile(a.win, sh, acc, MomentTaps{sxy});
    float sums[2] = {0.f, 0.f};   // S, |x - y|
    for_each_output(a.p, tl, [&](int o, int gy, int gx, int r, int c) {
        const float xv = sxy[0][r][c], yv = sxy[1][r][c];
        const SsimPixel px = ssim_pixel(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4]);
        sums[0] += px.s;
        sums[1] += fabsf(xv - yv);
        const size_t q = base + (size_t)gy * W + gx;
        if (kMap && a.ssim_map) a.ssim_map[q] = px.s;
        if (a.partials) {
            a.partials[q] = px.d_mu;
            a.partials[a.n + q] = px.d_exx;
            a.partials[2 * a.n + q] = px.d_exy;
        }
    });
    block_sums(sums, red);
    if (threadIdx.x == 0) {
        a.slots[blockIdx.x] = sums[0];
        a.slots[a.nblocks + blockIdx.x] = sums[1];
    }
}

__global__ __launch_bounds__(kBlock) void ssim_fwd_kernel(FwdArgs a)
{
    const int W = a.p.W;
    const Tile tl = tile_of(a.p);
    const size_t base = (size_t)tl.plane * a.p.H * W;
    const float* X = a.x + base;
    const float* Y = a.y + base;
    fwd_tile<true>(a, tl, base, [&](int gy, int gx, float (&v)[2]) {
        const size_t o = (size_t)gy * W + gx;
        v[0] = X[o];
        v[1] = Y[o];
    });
}

// |x - y| over a flat array (l1_loss of any shape): chunk sums into the L1 half of the slots, the S half zeroed
__global__ __launch_bounds__(kBlock) void l1_fwd_kernel(long long n, int nblocks, const float* __restrict__ x,
                                                        const float* __restrict__ y, float* __restrict__ slots)
{
    __shared__ float red[1][kBlock / 64];
    const long long b0 = (long long)blockIdx.x * kL1Chunk;
    float s[1] = {0.f};
#pragma unroll
    for (int i = 0; i < kL1Chunk / kBlock; i++) {
        const long long e = b0 + i * kBlock + threadIdx.x;
        if (e < n) s[0] += fabsf(x[e] - y[e]);
    }
    block_sums(s, red);
    if (threadIdx.x == 0) {
        slots[blockIdx.x] = 0.f;
        slots[nblocks + blockIdx.x] = s[0];
    }
}

struct ReduceArgs {
    int nimages, blocks_per_image, nblocks;
    double n_image, n_total;
    float lambda;
    const float* slots;
    float *l1_mean, *ssim_mean, *ssim_image, *loss, *dssim;
};

// One workgroup: per image, thread-strided double sums of its slots and a fixed tree; images in order.
__global__ __launch_bounds__(kBlock) void loss_reduce_kernel(ReduceArgs a)
{
    __shared__ double buf[2][kBlock];
    const int t = threadIdx.x;
    double tot_s = 0.0, tot_l = 0.0;
    for (int b = 0; b < a.nimages; b++) {
        const int first = b * a.blocks_per_image;
        const float* const run[2] = {a.slots + first, a.slots + a.nblocks + first};
        double sum[2];   // S, |x - y|
        slot_sums(run, a.blocks_per_image, sum, buf);
        if (t == 0 && a.ssim_image) a.ssim_image[b] = (float)(sum[0] / a.n_image);
        tot_s += sum[0];
        tot_l += sum[1];
    }
    if (t == 0) {
        const double l1 = tot_l / a.n_total, s = tot_s / a.n_total;
        if (a.l1_mean) a.l1_mean[0] = (float)l1;
        if (a.ssim_mean) a.ssim_mean[0] = (float)s;
        if (a.dssim) a.dssim[0] = (float)(1.0 - s);
        if (a.loss) a.loss[0] = (float)((1.0 - (double)a.lambda) * l1 + (double)a.lambda * (1.0 - s));
    }
}

struct BwdArgs {
    Plane p;
    int C;
    int mode;           // upstream gradient of S: 0 mean, 1 per image, 2 per pixel
    const float* x;
    const float* y;
    const float* partials;
    const float* g_l1;  // may be NULL
    const float* g_s;   // may be NULL
    float coef_l1, coef_s, inv_n, inv_image;
    float* dx;
    long long n;
    Window win;
};

// How a backward obtains the upstream gradient of S at element q.  GradSModes: r3dgs_l1_ssim_backward's, absent or in one of
// its three modes (`uniform` serves modes 0 and 1).  GradSUniform: one value everywhere (the exposed loss's scalar upstream).
struct GradSModes {
    const float* g_s;   // may be NULL: no SSIM term, the partial maps are not read
    int mode;
    float coef_s, uniform;
    __device__ bool present() const { return g_s; }
    __device__ float at(size_t q) const { return mode == 2 ? coef_s * g_s[q] : uniform; }
};

struct GradSUniform {
    float uniform;
    __device__ bool present() const { return true; }
    __device__ float at(size_t) const { return uniform; }
};

// One backward channel step on the plane at `base`: the three partial maps are staged, each scaled by the upstream gradient of
// S, and filtered; then pixel(o, q, g) is called at each of this thread's outputs (for_each_output's o, element q), where
// g(xv, yv) is the gradient with respect to xv of the pair (xv, yv) the forward staged there.  gl: the upstream gradient of |x - y|.
template <class GradS, class Pixel>
__device__ __forceinline__ void bwd_channel(const Plane& p, const Tile& tl, const Window& win, const float* partials, long long n,
                                            int plane, GradS gs, float gl, Pixel pixel)
{
    __shared__ float sq[3][kInH][kInW];
    __shared__ float sh[3][kInH][kTW];
    const int W = p.W;
    const size_t base = (size_t)plane * p.H * W;
    stage_tiles(p, tl, sq, [&](int gy, int gx, float (&v)[3]) {
        if (!gs.present()) return;
        const size_t q = base + (size_t)gy * W + gx;
        const float g = gs.at(q);
        v[0] = g * partials[q];
        v[1] = g * partials[n + q];
        v[2] = g * partials[2 * n + q];
    });
    float acc[kRows][3];
    filter_tile(win, sh, acc, [&](int r, int c, float (&v)[3]) {
#pragma unroll
        for (int m = 0; m < 3; m++) v[m] = sq[m][r][c];
    });
    for_each_output(p, tl, [&](int o, int gy, int gx, int, int) {
        const size_t pix = (size_t)gy * W + gx, q = base + pix;
        pixel(o, pix, q, [&](float xv, float yv) {
            const float ds = acc[o][0] + 2.f * xv * acc[o][1] + yv * acc[o][2];
            return gl * l1_sign(xv, yv) + ds;
        });
    });
}

// The backward of one workgroup per (plane, tile).  Args: BwdArgs or ExpBwdArgs (p, win, x, y, partials, n, dx).  kMasked:
// the forward staged (m x, m y or y), so the mask M of this plane's image (NULL: ones) multiplies x, y and dx.
template <bool kMasked, class Args, class GradS>
__device__ __forceinline__ void plane_bwd_tile(const Args& a, const Tile& tl, GradS gs, float gl, const float* M = nullptr,
                                               bool mask_target = false)
{
    bwd_channel(a.p, tl, a.win, a.partials, a.n, tl.plane, gs, gl, [&](int, size_t pix, size_t q, auto g) {
        if constexpr (kMasked) {
            const float m = M ? M[pix] : 1.f;
            const float xv = m * a.x[q], yv = mask_target ? m * a.y[q] : a.y[q];
            a.dx[q] = m * g(xv, yv);
        } else {
            a.dx[q] = g(a.x[q], a.y[q]);
        }
    });
}

__global__ __launch_bounds__(kBlock) void ssim_bwd_kernel(BwdArgs a)
{
    const Tile tl = tile_of(a.p);
    // upstream gradient of S: uniform for modes 0 and 1
    float gs_uniform = 0.f;
    if (a.g_s && a.mode == 0) gs_uniform = a.coef_s * a.g_s[0] * a.inv_n;
    if (a.g_s && a.mode == 1) gs_uniform = a.coef_s * a.g_s[tl.plane / a.C] * a.inv_image;
    const float gl = a.g_l1 ? a.coef_l1 * a.g_l1[0] * a.inv_n : 0.f;
    plane_bwd_tile<false>(a, tl, GradSModes{a.g_s, a.mode, a.coef_s, gs_uniform}, gl);
}

__global__ __launch_bounds__(kBlock) void l1_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ grad, float inv_n, float* __restrict__ dx)
{
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    dx[e] = grad[0] * inv_n * r3::l1_sign(x[e], y[e]);
}

long long ssim_blocks(int B, int C, int H, int W)
{
    return B < 1 || C < 1 ? -1 : tile_blocks((long long)B * C, H, W);
}

// -> the tile kernels' workgroups; `what` names the refusing entry point(s)
long long check_shape(const char* what, int B, int C, int H, int W)
{
    const long long nb = ssim_blocks(B, C, H, W);
    if (nb < 0)
        throw r3::Error(std::string(what) + ": need B, C, H, W >= 1 and fewer than 2^31 tiles, got " + std::to_string(B) + "x" +
                        std::to_string(C) + "x" + std::to_string(H) + "x" + std::to_string(W));
    return nb;
}

// ---- the same loss behind a per-image exposure and a pixel mask (r3dgs_exposure_loss_*): x'' = m (x E[:, :3] + E[:, 3]),
// y' = m y or y (exposure_math.h).  The forward stages (x'', y') instead of (x, y); the backward recomputes x'' and y' where
// the plain one reads x and y, and carries the gradient of x'' on to x and to E.

struct ExposureIn {
    const float* E;      // [B or 1][3][4], or NULL: identity
    const float* mask;   // [B or 1][H][W], or NULL: ones
    int e_per_image, mask_per_image, mask_target;
};

struct ExpFwdArgs {
    FwdArgs f;   // x, y: the inputs before the map; ssim_map unused
    int C;
    ExposureIn in;
};

__global__ __launch_bounds__(kBlock) void exposure_fwd_kernel(ExpFwdArgs a)
{
    const int W = a.f.p.W;
    const Tile tl = tile_of(a.f.p);
    const size_t hw = (size_t)a.f.p.H * W;
    const size_t base = (size_t)tl.plane * hw;
    const int b = tl.plane / a.C, ch = tl.plane - b * a.C;
    const float* Y = a.f.y + base;
    const float* M = a.in.mask ? a.in.mask + (a.in.mask_per_image ? (size_t)b * hw : 0) : nullptr;
    // this channel's own plane (the diagonal term) and, under an exposure, the other two in rising order with their coefficients
    const float* Xd = a.f.x + base;
    const float *Xa = Xd, *Xb = Xd;
    float ed = 1.f, ea = 0.f, eb = 0.f, off = 0.f;
    if (a.in.E) {
        const float* E = a.in.E + (a.in.e_per_image ? (size_t)b * kExposureFloats : 0);
        const int ka = exposure_other_a(ch), kb = exposure_other_b(ch);
        Xa = a.f.x + ((size_t)b * 3 + ka) * hw;
        Xb = a.f.x + ((size_t)b * 3 + kb) * hw;
        ed = E[4 * ch + ch];
        ea = E[4 * ka + ch];
        eb = E[4 * kb + ch];
        off = E[4 * ch + 3];
    }
    fwd_tile<false>(a.f, tl, base, [&](int gy, int gx, float (&v)[2]) {
        const size_t o = (size_t)gy * W + gx;
        const float m = M ? M[o] : 1.f;
        const float yv = Y[o];
        v[0] = a.in.E ? exposure_sum(ed, ea, eb, off, Xd[o], Xa[o], Xb[o], m) : m * Xd[o];
        v[1] = a.in.mask_target ? m * yv : yv;
    });
}

struct ExpBwdArgs {
    Plane p;
    int C;
    const float* x;
    const float* y;
    const float* partials;
    const float* g;     // upstream gradient of the loss, [1]
    float coef_l1, coef_s, inv_n;
    ExposureIn in;
    float* dx;
    double* slots;      // [12][nslots] per-workgroup sums of dE, or NULL: dE not wanted
    int nslots;
    long long n;
    Window win;
};

// No exposure (any C): one workgroup per (plane, tile) as the plain backward, with x'' = m x, y' = m y or y, dx = m g.
__global__ __launch_bounds__(kBlock) void masked_bwd_kernel(ExpBwdArgs a)
{
    const Tile tl = tile_of(a.p);
    const size_t hw = (size_t)a.p.H * a.p.W;
    const float* M = a.in.mask ? a.in.mask + (a.in.mask_per_image ? (size_t)(tl.plane / a.C) * hw : 0) : nullptr;
    const float gs_uniform = a.coef_s * a.g[0] * a.inv_n;
    const float gl = a.coef_l1 * a.g[0] * a.inv_n;
    plane_bwd_tile<true>(a, tl, GradSUniform{gs_uniform}, gl, M, a.in.mask_target);
}

// Under an exposure (C = 3): one workgroup per (image, tile).  Per channel the scaled partials are staged and filtered and
// g_c = dL/dx''_c formed from the recomputed x''_c and y'_c; the kRows x 3 values of g stay in registers, then dx_k of the three
// planes is written and the twelve terms of dE summed per thread in double, per workgroup into its slots (fixed order).
__global__ __launch_bounds__(kBlock) void exposure_bwd_kernel(ExpBwdArgs a)
{
    __shared__ double red[kExposureFloats][kBlock / 64];
    const int W = a.p.W;
    const Tile tl = tile_of(a.p);   // .plane: the image
    const size_t hw = (size_t)a.p.H * W;
    const size_t ibase = (size_t)tl.plane * 3 * hw;
    const float* M = a.in.mask ? a.in.mask + (a.in.mask_per_image ? (size_t)tl.plane * hw : 0) : nullptr;
    const float* Eg = a.in.E + (a.in.e_per_image ? (size_t)tl.plane * kExposureFloats : 0);
    float E[kExposureFloats];
#pragma unroll
    for (int i = 0; i < kExposureFloats; i++) E[i] = Eg[i];
    const float gs_uniform = a.coef_s * a.g[0] * a.inv_n;
    const float gl = a.coef_l1 * a.g[0] * a.inv_n;
    float xin[kRows][3], mv[kRows], g[kRows][3];
#pragma unroll
    for (int o = 0; o < kRows; o++) {
        mv[o] = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) xin[o][k] = g[o][k] = 0.f;
    }
    for_each_output(a.p, tl, [&](int o, int gy, int gx, int, int) {
        const size_t q = (size_t)gy * W + gx;
        mv[o] = M ? M[q] : 1.f;
#pragma unroll
        for (int k = 0; k < 3; k++) xin[o][k] = a.x[ibase + k * hw + q];
    });
#pragma unroll
    for (int c = 0; c < 3; c++) {
        bwd_channel(a.p, tl, a.win, a.partials, a.n, tl.plane * 3 + c, GradSUniform{gs_uniform}, gl, [&](int o, size_t, size_t q, auto gc) {
            const float xv = exposed(E, xin[o][0], xin[o][1], xin[o][2], mv[o], c);
            const float yv = a.in.mask_target ? mv[o] * a.y[q] : a.y[q];
            g[o][c] = gc(xv, yv);
        });
    }
    double dE[kExposureFloats];
#pragma unroll
    for (int i = 0; i < kExposureFloats; i++) dE[i] = 0.0;
    for_each_output(a.p, tl, [&](int o, int gy, int gx, int, int) {
        const size_t q = ibase + (size_t)gy * W + gx;
#pragma unroll
        for (int k = 0; k < 3; k++) a.dx[q + k * hw] = exposed_adjoint(E, g[o][0], g[o][1], g[o][2], mv[o], k);
        if (a.slots) exposure_grad_accumulate(dE, xin[o][0], xin[o][1], xin[o][2], g[o][0], g[o][1], g[o][2], mv[o]);
    });
    if (!a.slots) return;
    block_sums(dE, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kExposureFloats; i++) a.slots[(size_t)i * a.nslots + blockIdx.x] = dE[i];
    }
}

struct ExpFinishArgs {
    int B, tiles, shared;
    const double* slots;   // [12][B * tiles]
    float* dE;             // [B][3][4], or [3][4] when shared
};

// One workgroup: each of the twelve entries, image by image, thread-strided double sums of its slots and a fixed tree; a shared
// exposure gets the sum over the images in their order.
__global__ __launch_bounds__(kBlock) void exposure_finish_kernel(ExpFinishArgs a)
{
    __shared__ double buf[1][kBlock];
    const int t = threadIdx.x;
    const size_t nslots = (size_t)a.B * a.tiles;
    for (int i = 0; i < kExposureFloats; i++) {
        double total = 0.0;
        for (int b = 0; b < a.B; b++) {
            const double* const run[1] = {a.slots + i * nslots + (size_t)b * a.tiles};
            double s[1];
            slot_sums(run, a.tiles, s, buf);
            total += s[0];
            if (t == 0 && !a.shared) a.dE[b * kExposureFloats + i] = (float)s[0];
        }
        if (t == 0 && a.shared) a.dE[i] = (float)total;
    }
}

// out = clamp?(x E[:, :3] + E[:, 3]) per pixel: evaluation and saving (train_test_exp); no gradient
__global__ __launch_bounds__(kBlock) void exposure_apply_kernel(long long npix, long long hw, const float* __restrict__ img,
                                                                const float* __restrict__ exposure, int e_per_image, int clamp01,
                                                                float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (p >= npix) return;
    const long long b = p / hw, q = b * 3 * hw + (p - b * hw);
    const float* E = exposure + (e_per_image ? b * kExposureFloats : 0);
    const float x0 = img[q], x1 = img[q + hw], x2 = img[q + 2 * hw];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = exposed(E, x0, x1, x2, 1.f, c);
        if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
        out[q + c * hw] = v;
    }
}

// byte offsets in the exposure loss's workspace: the forward's float slots [2][B*C*tiles], then the backward's double slots
// [12][B*tiles]
struct ExpWorkspace {
    long long nblocks, image_tiles;   // B*C*tiles, B*tiles; nblocks < 0: invalid shape
    size_t dE_offset, bytes;
};

ExpWorkspace exposure_workspace(int B, int C, int H, int W)
{
    ExpWorkspace w{};
    w.nblocks = ssim_blocks(B, C, H, W);
    if (w.nblocks < 0) return w;
    w.image_tiles = w.nblocks / C;
    w.dE_offset = (size_t)(2 * w.nblocks) * sizeof(float);
    w.bytes = w.dE_offset + (size_t)(kExposureFloats * w.image_tiles) * sizeof(double);
    return w;
}

// what both exposure loss calls refuse -> the workspace layout
ExpWorkspace check_exposure_call(const char* what, int B, int C, int H, int W, const float* exposure, const char* workspace,
                                 size_t workspace_bytes)
{
    const std::string name(what);
    check_shape(what, B, C, H, W);
    const ExpWorkspace w = exposure_workspace(B, C, H, W);
    if (exposure && C != 3)
        throw r3::Error(name + ": an exposure maps 3 colour channels, the images have C = " + std::to_string(C));
    if (!workspace) throw r3::Error(name + ": a required pointer is NULL");
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double) != 0)
        throw r3::Error(name + ": the workspace must be 8-byte aligned (it holds double sums)");
    if (workspace_bytes < w.bytes)
        throw r3::Error(name + ": the workspace holds " + std::to_string(workspace_bytes) + " bytes, this shape needs " +
                        std::to_string(w.bytes) + " (r3dgs_exposure_loss_workspace_bytes)");
    return w;
}

// the tile forward's arguments, of a shape check_shape accepts
FwdArgs fwd_args(int B, int C, int H, int W, const float* x, const float* y, float* partials, float* ssim_map, char* workspace)
{
    FwdArgs a;
    a.p = plane_of(H, W);
    a.nblocks = (int)ssim_blocks(B, C, H, W);
    a.x = x;
    a.y = y;
    a.ssim_map = ssim_map;
    a.partials = partials;
    a.slots = reinterpret_cast<float*>(workspace);
    a.n = (long long)B * C * H * W;
    a.win = window();
    return a;
}

// loss_reduce_kernel over the slots [2][nimages * blocks_per_image] a forward left, each image of n_image elements; an output
// that is NULL is not written
void launch_reduce(hipStream_t s, int nimages, int blocks_per_image, double n_image, float lambda, const float* slots,
                   float* l1_mean, float* ssim_mean, float* ssim_image, float* loss, float* dssim)
{
    const ReduceArgs r{nimages, blocks_per_image, nimages * blocks_per_image, n_image, nimages * n_image, lambda, slots,
                       l1_mean, ssim_mean, ssim_image, loss, dssim};
    loss_reduce_kernel<<<1, kBlock, 0, s>>>(r);
    r3::check_launch("loss reduce", s, false);
}

}  // namespace

extern "C" {

void r3dgs_ssim_window(float w[11])
{
    for (int i = 0; i < kSsimTaps; i++) w[i] = window().w[i];
}

size_t r3dgs_l1_ssim_workspace_bytes(int B, int C, int H, int W)
{
    const long long nb = ssim_blocks(B, C, H, W);
    return nb < 0 ? 0 : (size_t)(2 * nb) * sizeof(float);
}

int r3dgs_l1_ssim_forward(int B, int C, int H, int W, const float* img1, const float* img2, float lambda_dssim,
                          float* l1_mean, float* ssim_mean, float* ssim_image, float* loss, float* dssim, float* ssim_map,
                          float* partials, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        check_shape("l1_ssim", B, C, H, W);
        if (!img1 || !img2 || !workspace) throw r3::Error("l1_ssim_forward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const FwdArgs a = fwd_args(B, C, H, W, img1, img2, partials, ssim_map, workspace);
        ssim_fwd_kernel<<<a.nblocks, kBlock, 0, s>>>(a);
        r3::check_launch("ssim forward", s, false);
        launch_reduce(s, B, C * a.p.tiles_per_plane, (double)C * H * W, lambda_dssim, a.slots, l1_mean, ssim_mean, ssim_image,
                      loss, dssim);
        return 0;
    });
}

int r3dgs_l1_ssim_backward(int B, int C, int H, int W, const float* img1, const float* img2, const float* partials,
                           const float* grad_l1, float coef_l1, const float* grad_ssim, int ssim_grad_mode, float coef_ssim,
                           float* grad_img1, void* stream)
{
    return r3::guarded_call([&]() {
        const long long nb = check_shape("l1_ssim", B, C, H, W);
        if (!img1 || !img2 || !grad_img1) throw r3::Error("l1_ssim_backward: a required pointer is NULL");
        if (grad_ssim && !partials) throw r3::Error("l1_ssim_backward: the SSIM gradient needs the forward's partial maps");
        if (ssim_grad_mode < 0 || ssim_grad_mode > 2) throw r3::Error("l1_ssim_backward: ssim_grad_mode must be 0, 1 or 2");
        hipStream_t s = static_cast<hipStream_t>(stream);
        BwdArgs a;
        a.p = plane_of(H, W);
        a.C = C;
        a.mode = ssim_grad_mode;
        a.x = img1;
        a.y = img2;
        a.partials = partials;
        a.g_l1 = grad_l1;
        a.g_s = grad_ssim;
        a.coef_l1 = coef_l1;
        a.coef_s = coef_ssim;
        a.n = (long long)B * C * H * W;
        a.inv_n = (float)(1.0 / (double)a.n);
        a.inv_image = (float)(1.0 / ((double)C * H * W));
        a.dx = grad_img1;
        a.win = window();
        ssim_bwd_kernel<<<(int)nb, kBlock, 0, s>>>(a);
        r3::check_launch("ssim backward", s, false);
        return 0;
    });
}

size_t r3dgs_l1_workspace_bytes(long long n)
{
    if (n < 1 || (n + kL1Chunk - 1) / kL1Chunk > 0x7fffffffLL) return 0;
    return (size_t)(2 * ((n + kL1Chunk - 1) / kL1Chunk)) * sizeof(float);
}

int r3dgs_l1_forward(long long n, const float* x, const float* y, float* l1_mean, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        if (r3dgs_l1_workspace_bytes(n) == 0) throw r3::Error("l1_forward: need 1 <= n < 2^41 elements");
        if (!x || !y || !workspace) throw r3::Error("l1_forward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const int nb = (int)((n + kL1Chunk - 1) / kL1Chunk);
        float* slots = reinterpret_cast<float*>(workspace);
        l1_fwd_kernel<<<nb, kBlock, 0, s>>>(n, nb, x, y, slots);
        r3::check_launch("l1 forward", s, false);
        launch_reduce(s, 1, nb, (double)n, 0.f, slots, l1_mean, nullptr, nullptr, nullptr, nullptr);
        return 0;
    });
}

int r3dgs_l1_backward(long long n, const float* x, const float* y, const float* grad, float* grad_x, void* stream)
{
    return r3::guarded_call([&]() {
        if (n < 1 || (n + kBlock - 1) / kBlock > 0x7fffffffLL) throw r3::Error("l1_backward: need 1 <= n < 2^39 elements");
        if (!x || !y || !grad || !grad_x) throw r3::Error("l1_backward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        l1_bwd_kernel<<<(int)((n + kBlock - 1) / kBlock), kBlock, 0, s>>>(n, x, y, grad, (float)(1.0 / (double)n), grad_x);
        r3::check_launch("l1 backward", s, false);
        return 0;
    });
}

size_t r3dgs_exposure_loss_workspace_bytes(int B, int C, int H, int W)
{
    return exposure_workspace(B, C, H, W).bytes;
}

int r3dgs_exposure_loss_forward(int B, int C, int H, int W, const float* img1, const float* img2, const float* exposure,
                                int exposure_per_image, const float* mask, int mask_per_image, int mask_target,
                                float lambda_dssim, float* l1_mean, float* ssim_mean, float* ssim_image, float* loss,
                                float* dssim, float* partials, char* workspace, size_t workspace_bytes, void* stream)
{
    return r3::guarded_call([&]() {
        check_exposure_call("exposure_loss_forward", B, C, H, W, exposure, workspace, workspace_bytes);
        if (!img1 || !img2) throw r3::Error("exposure_loss_forward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        const ExpFwdArgs a{fwd_args(B, C, H, W, img1, img2, partials, nullptr, workspace), C,
                           ExposureIn{exposure, mask, exposure_per_image != 0, mask_per_image != 0, mask_target != 0}};
        exposure_fwd_kernel<<<a.f.nblocks, kBlock, 0, s>>>(a);
        r3::check_launch("exposure loss forward", s, false);
        launch_reduce(s, B, C * a.f.p.tiles_per_plane, (double)C * H * W, lambda_dssim, a.f.slots, l1_mean, ssim_mean, ssim_image,
                      loss, dssim);
        return 0;
    });
}

int r3dgs_exposure_loss_backward(int B, int C, int H, int W, const float* img1, const float* img2, const float* exposure,
                                 int exposure_per_image, const float* mask, int mask_per_image, int mask_target,
                                 const float* partials, const float* grad_loss, float coef_l1, float coef_ssim,
                                 float* grad_img1, float* grad_exposure, char* workspace, size_t workspace_bytes, void* stream)
{
    return r3::guarded_call([&]() {
        const ExpWorkspace w = check_exposure_call("exposure_loss_backward", B, C, H, W, exposure, workspace, workspace_bytes);
        if (!img1 || !img2 || !partials || !grad_loss || !grad_img1)
            throw r3::Error("exposure_loss_backward: a required pointer is NULL");
        if (grad_exposure && !exposure)
            throw r3::Error("exposure_loss_backward: grad_exposure is asked for without an exposure");
        hipStream_t s = static_cast<hipStream_t>(stream);
        ExpBwdArgs a;
        a.p = plane_of(H, W);
        a.C = C;
        a.x = img1;
        a.y = img2;
        a.partials = partials;
        a.g = grad_loss;
        a.coef_l1 = coef_l1;
        a.coef_s = coef_ssim;
        a.n = (long long)B * C * H * W;
        a.inv_n = (float)(1.0 / (double)a.n);
        a.in = ExposureIn{exposure, mask, exposure_per_image != 0, mask_per_image != 0, mask_target != 0};
        a.dx = grad_img1;
        a.slots = grad_exposure ? reinterpret_cast<double*>(workspace + w.dE_offset) : nullptr;
        a.nslots = (int)w.image_tiles;
        a.win = window();
        if (!exposure) {
            masked_bwd_kernel<<<(int)w.nblocks, kBlock, 0, s>>>(a);
            r3::check_launch("masked loss backward", s, false);
            return 0;
        }
        exposure_bwd_kernel<<<(int)w.image_tiles, kBlock, 0, s>>>(a);
        r3::check_launch("exposure loss backward", s, false);
        if (grad_exposure) {
            ExpFinishArgs f;
            f.B = B;
            f.tiles = a.p.tiles_per_plane;
            f.shared = !exposure_per_image;
            f.slots = a.slots;
            f.dE = grad_exposure;
            exposure_finish_kernel<<<1, kBlock, 0, s>>>(f);
            r3::check_launch("exposure gradient finish", s, false);
        }
        return 0;
    });
}

int r3dgs_exposure_apply(int B, int H, int W, const float* img, const float* exposure, int exposure_per_image, int clamp01,
                         float* out, void* stream)
{
    return r3::guarded_call([&]() {
        const long long hw = (long long)H * W, npix = hw * B;
        if (B < 1 || H < 1 || W < 1 || (npix + kBlock - 1) / kBlock > 0x7fffffffLL)
            throw r3::Error("exposure_apply: need B, H, W >= 1 and fewer than 2^39 pixels, got " + std::to_string(B) + "x3x" +
                            std::to_string(H) + "x" + std::to_string(W));
        if (!img || !exposure || !out) throw r3::Error("exposure_apply: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        exposure_apply_kernel<<<(int)((npix + kBlock - 1) / kBlock), kBlock, 0, s>>>(npix, hw, img, exposure,
                                                                                    exposure_per_image != 0, clamp01 != 0, out);
        r3::check_launch("exposure apply", s, false);
        return 0;
    });
}

}  // extern "C"
