// loss.hip -- the fused L1 + D-SSIM training loss (include/r3dgs_loss.h), forward and backward.
//
// What the reference does (utils/loss_utils.py:17-66, train.py:109-115): five 11x11 depthwise F.conv2d calls with zero
// padding 5 (mu_x, mu_y, E[x^2], E[y^2], E[xy]), about fifteen elementwise ops and autograd's backward of all of them --
// ~15 full-size intermediate maps forward and twice as many backward.  How it is issued here:
//   * forward: one workgroup per 64 x 16 output tile of one (image, channel) plane.  x and y are staged with their 5-pixel
//     halo in LDS (zeros outside the image), the five moments are filtered horizontally into LDS and then vertically in
//     registers (separable window, the reference's fp32 1-D weights), and per pixel loss_math.h gives S and its three
//     partials.  The workgroup writes its sums of S and |x - y| to its own workspace slot; in training mode it also
//     writes the three partial maps (12 B per element), optionally the S map.
//   * reduction: one workgroup adds the slots of each image in a fixed order (double accumulators) and writes the means,
//     the per-image means and the combined loss.
//   * backward: the same tiling over the three partial maps, each scaled by the upstream gradient of S at its pixel; the
//     transpose of a zero-padded convolution with a symmetric window is the same filter over in-image positions, so
//     dx = F[gS dS/dmu_x] + 2x F[gS dS/dE_xx] + y F[gS dS/dE_xy] + g_l1 sign(x - y) / n.
// No atomics anywhere: every sum has a fixed order, so values and gradients are identical run to run.
#include "../../include/r3dgs_loss.h"

#include <cmath>

#include "common.h"
#include "loss_math.h"

namespace {

using r3::kSsimRadius;
using r3::kSsimTaps;

constexpr int kBlock = 256;
constexpr int kTW = 64;                     // tile width: one wave spans a tile row
constexpr int kTH = 16;                     // tile height
constexpr int kRows = kTH / (kBlock / kTW); // output rows per thread (4)
constexpr int kInW = kTW + 2 * kSsimRadius; // staged width with halo (74)
constexpr int kInH = kTH + 2 * kSsimRadius; // staged height with halo (26)
constexpr int kL1Chunk = 4 * kBlock;        // elements per workgroup of the flat L1 kernel

struct Window {
    float w[kSsimTaps];
};

struct Plane {
    int H, W, tiles_x, tiles_per_plane;
};

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Two block-wide sums in a fixed order; thread 0 gets the results.
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[kBlock / 64])
{
    a = wave_sum(a);
    b = wave_sum(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = a;
        red[1][wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

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

__global__ __launch_bounds__(kBlock) void ssim_fwd_kernel(FwdArgs a)
{
    __shared__ float sx[kInH][kInW], sy[kInH][kInW];
    __shared__ float sh[5][kInH][kTW];
    __shared__ float red[2][kBlock / 64];
    const int t = threadIdx.x, H = a.p.H, W = a.p.W;
    const int plane = blockIdx.x / a.p.tiles_per_plane, tile = blockIdx.x - plane * a.p.tiles_per_plane;
    const int ty = tile / a.p.tiles_x, tx = tile - ty * a.p.tiles_x;
    const int gx0 = tx * kTW, gy0 = ty * kTH;
    const size_t base = (size_t)plane * H * W;
    const float* X = a.x + base;
    const float* Y = a.y + base;
    for (int e = t; e < kInH * kInW; e += kBlock) {
        const int r = e / kInW, c = e - r * kInW;
        const int gy = gy0 - kSsimRadius + r, gx = gx0 - kSsimRadius + c;
        float vx = 0.f, vy = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t o = (size_t)gy * W + gx;
            vx = X[o];
            vy = Y[o];
        }
        sx[r][c] = vx;
        sy[r][c] = vy;
    }
    __syncthreads();
    const int c = t & (kTW - 1), rg = t / kTW;
    // horizontal pass of the five moments: (kInH rows) x (kTW columns)
    for (int r = rg; r < kInH; r += kBlock / kTW) {
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < kSsimTaps; k++) {
            const float w = a.win.w[k], xv = sx[r][c + k], yv = sy[r][c + k];
            m1 = fmaf(w, xv, m1);
            m2 = fmaf(w, yv, m2);
            e11 = fmaf(w, xv * xv, e11);
            e22 = fmaf(w, yv * yv, e22);
            e12 = fmaf(w, xv * yv, e12);
        }
        sh[0][r][c] = m1;
        sh[1][r][c] = m2;
        sh[2][r][c] = e11;
        sh[3][r][c] = e22;
        sh[4][r][c] = e12;
    }
    __syncthreads();
    // vertical pass: this thread's kRows consecutive output rows of column c
    const int r0 = rg * kRows;
    float acc[kRows][5];
#pragma unroll
    for (int o = 0; o < kRows; o++)
#pragma unroll
        for (int m = 0; m < 5; m++) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < kRows + 2 * kSsimRadius; j++) {
        float v[5];
#pragma unroll
        for (int m = 0; m < 5; m++) v[m] = sh[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < kRows; o++) {
            const int k = j - o;
            if (k >= 0 && k < kSsimTaps) {
#pragma unroll
                for (int m = 0; m < 5; m++) acc[o][m] = fmaf(a.win.w[k], v[m], acc[o][m]);
            }
        }
    }
    float sum_s = 0.f, sum_l1 = 0.f;
    const int gx = gx0 + c;
#pragma unroll
    for (int o = 0; o < kRows; o++) {
        const int gy = gy0 + r0 + o;
        if (gx >= W || gy >= H) continue;
        const float xv = sx[r0 + o + kSsimRadius][c + kSsimRadius], yv = sy[r0 + o + kSsimRadius][c + kSsimRadius];
        const r3::SsimPixel px = r3::ssim_pixel(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4]);
        sum_s += px.s;
        sum_l1 += fabsf(xv - yv);
        const size_t q = base + (size_t)gy * W + gx;
        if (a.ssim_map) a.ssim_map[q] = px.s;
        if (a.partials) {
            a.partials[q] = px.d_mu;
            a.partials[a.n + q] = px.d_exx;
            a.partials[2 * a.n + q] = px.d_exy;
        }
    }
    block_sum2(sum_s, sum_l1, red);
    if (t == 0) {
        a.slots[blockIdx.x] = sum_s;
        a.slots[a.nblocks + blockIdx.x] = sum_l1;
    }
}

// |x - y| over a flat array (l1_loss of any shape): chunk sums into the L1 half of the slots, the S half zeroed
__global__ __launch_bounds__(kBlock) void l1_fwd_kernel(long long n, int nblocks, const float* __restrict__ x,
                                                        const float* __restrict__ y, float* __restrict__ slots)
{
    __shared__ float red[2][kBlock / 64];
    const long long b0 = (long long)blockIdx.x * kL1Chunk;
    float s = 0.f, zero = 0.f;
#pragma unroll
    for (int i = 0; i < kL1Chunk / kBlock; i++) {
        const long long e = b0 + i * kBlock + threadIdx.x;
        if (e < n) s += fabsf(x[e] - y[e]);
    }
    block_sum2(zero, s, red);
    if (threadIdx.x == 0) {
        slots[blockIdx.x] = 0.f;
        slots[nblocks + blockIdx.x] = s;
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
    __shared__ double rs[kBlock], rl[kBlock];
    const int t = threadIdx.x;
    double tot_s = 0.0, tot_l = 0.0;
    for (int b = 0; b < a.nimages; b++) {
        double s = 0.0, l = 0.0;
        const int first = b * a.blocks_per_image;
        for (int i = t; i < a.blocks_per_image; i += kBlock) {
            s += a.slots[first + i];
            l += a.slots[a.nblocks + first + i];
        }
        rs[t] = s;
        rl[t] = l;
        __syncthreads();
        for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
            if (t < stride) {
                rs[t] += rs[t + stride];
                rl[t] += rl[t + stride];
            }
            __syncthreads();
        }
        if (t == 0) {
            if (a.ssim_image) a.ssim_image[b] = (float)(rs[0] / a.n_image);
            tot_s += rs[0];
            tot_l += rl[0];
        }
        __syncthreads();
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

__global__ __launch_bounds__(kBlock) void ssim_bwd_kernel(BwdArgs a)
{
    __shared__ float sq[3][kInH][kInW];
    __shared__ float sh[3][kInH][kTW];
    const int t = threadIdx.x, H = a.p.H, W = a.p.W;
    const int plane = blockIdx.x / a.p.tiles_per_plane, tile = blockIdx.x - plane * a.p.tiles_per_plane;
    const int ty = tile / a.p.tiles_x, tx = tile - ty * a.p.tiles_x;
    const int gx0 = tx * kTW, gy0 = ty * kTH;
    const size_t base = (size_t)plane * H * W;
    // upstream gradient of S: uniform for modes 0 and 1
    float gs_uniform = 0.f;
    if (a.g_s && a.mode == 0) gs_uniform = a.coef_s * a.g_s[0] * a.inv_n;
    if (a.g_s && a.mode == 1) gs_uniform = a.coef_s * a.g_s[plane / a.C] * a.inv_image;
    const float gl = a.g_l1 ? a.coef_l1 * a.g_l1[0] * a.inv_n : 0.f;
    for (int e = t; e < kInH * kInW; e += kBlock) {
        const int r = e / kInW, c = e - r * kInW;
        const int gy = gy0 - kSsimRadius + r, gx = gx0 - kSsimRadius + c;
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
        if (a.g_s && gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t q = base + (size_t)gy * W + gx;
            const float g = a.mode == 2 ? a.coef_s * a.g_s[q] : gs_uniform;
            q0 = g * a.partials[q];
            q1 = g * a.partials[a.n + q];
            q2 = g * a.partials[2 * a.n + q];
        }
        sq[0][r][c] = q0;
        sq[1][r][c] = q1;
        sq[2][r][c] = q2;
    }
    __syncthreads();
    const int c = t & (kTW - 1), rg = t / kTW;
    for (int r = rg; r < kInH; r += kBlock / kTW) {
        float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
        for (int k = 0; k < kSsimTaps; k++) {
            const float w = a.win.w[k];
            h0 = fmaf(w, sq[0][r][c + k], h0);
            h1 = fmaf(w, sq[1][r][c + k], h1);
            h2 = fmaf(w, sq[2][r][c + k], h2);
        }
        sh[0][r][c] = h0;
        sh[1][r][c] = h1;
        sh[2][r][c] = h2;
    }
    __syncthreads();
    const int r0 = rg * kRows;
    float acc[kRows][3];
#pragma unroll
    for (int o = 0; o < kRows; o++)
#pragma unroll
        for (int m = 0; m < 3; m++) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < kRows + 2 * kSsimRadius; j++) {
        float v[3];
#pragma unroll
        for (int m = 0; m < 3; m++) v[m] = sh[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < kRows; o++) {
            const int k = j - o;
            if (k >= 0 && k < kSsimTaps) {
#pragma unroll
                for (int m = 0; m < 3; m++) acc[o][m] = fmaf(a.win.w[k], v[m], acc[o][m]);
            }
        }
    }
    const int gx = gx0 + c;
#pragma unroll
    for (int o = 0; o < kRows; o++) {
        const int gy = gy0 + r0 + o;
        if (gx >= W || gy >= H) continue;
        const size_t q = base + (size_t)gy * W + gx;
        const float xv = a.x[q], yv = a.y[q];
        const float ds = acc[o][0] + 2.f * xv * acc[o][1] + yv * acc[o][2];
        a.dx[q] = gl * r3::l1_sign(xv, yv) + ds;
    }
}

__global__ __launch_bounds__(kBlock) void l1_bwd_kernel(long long n, const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ grad, float inv_n, float* __restrict__ dx)
{
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    dx[e] = grad[0] * inv_n * r3::l1_sign(x[e], y[e]);
}

// utils/loss_utils.py:24-26: torch.Tensor([exp(...)]) rounds each double to fp32; gauss.sum() of the 11 fp32 values
// rounds to the same fp32 as their exact sum (checked bit for bit against the reference in tests/test_loss_cpu.py)
Window make_window()
{
    Window w;
    double sum = 0.0;
    for (int i = 0; i < kSsimTaps; i++) {
        const double d = i - kSsimRadius;
        w.w[i] = (float)std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += w.w[i];
    }
    const float fsum = (float)sum;
    for (int i = 0; i < kSsimTaps; i++) w.w[i] = w.w[i] / fsum;
    return w;
}

const Window& window()
{
    static const Window w = make_window();
    return w;
}

Plane plane_of(int H, int W)
{
    Plane p;
    p.H = H;
    p.W = W;
    p.tiles_x = (W + kTW - 1) / kTW;
    p.tiles_per_plane = p.tiles_x * ((H + kTH - 1) / kTH);
    return p;
}

long long ssim_blocks(int B, int C, int H, int W)
{
    if (B < 1 || C < 1 || H < 1 || W < 1) return -1;
    const long long nb = (long long)B * C * plane_of(H, W).tiles_per_plane;
    return nb > 0x7fffffffLL ? -1 : nb;
}

void check_shape(int B, int C, int H, int W)
{
    if (ssim_blocks(B, C, H, W) < 0)
        throw r3::Error("l1_ssim: need B, C, H, W >= 1 and fewer than 2^31 tiles, got " + std::to_string(B) + "x" +
                        std::to_string(C) + "x" + std::to_string(H) + "x" + std::to_string(W));
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
        check_shape(B, C, H, W);
        if (!img1 || !img2 || !workspace) throw r3::Error("l1_ssim_forward: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        FwdArgs a;
        a.p = plane_of(H, W);
        a.nblocks = (int)ssim_blocks(B, C, H, W);
        a.x = img1;
        a.y = img2;
        a.ssim_map = ssim_map;
        a.partials = partials;
        a.slots = reinterpret_cast<float*>(workspace);
        a.n = (long long)B * C * H * W;
        a.win = window();
        ssim_fwd_kernel<<<a.nblocks, kBlock, 0, s>>>(a);
        r3::check_launch("ssim forward", s, false);
        ReduceArgs r;
        r.nimages = B;
        r.blocks_per_image = C * a.p.tiles_per_plane;
        r.nblocks = a.nblocks;
        r.n_image = (double)C * H * W;
        r.n_total = (double)a.n;
        r.lambda = lambda_dssim;
        r.slots = a.slots;
        r.l1_mean = l1_mean;
        r.ssim_mean = ssim_mean;
        r.ssim_image = ssim_image;
        r.loss = loss;
        r.dssim = dssim;
        loss_reduce_kernel<<<1, kBlock, 0, s>>>(r);
        r3::check_launch("loss reduce", s, false);
        return 0;
    });
}

int r3dgs_l1_ssim_backward(int B, int C, int H, int W, const float* img1, const float* img2, const float* partials,
                           const float* grad_l1, float coef_l1, const float* grad_ssim, int ssim_grad_mode, float coef_ssim,
                           float* grad_img1, void* stream)
{
    return r3::guarded_call([&]() {
        check_shape(B, C, H, W);
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
        ssim_bwd_kernel<<<(int)ssim_blocks(B, C, H, W), kBlock, 0, s>>>(a);
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
        ReduceArgs r{};
        r.nimages = 1;
        r.blocks_per_image = nb;
        r.nblocks = nb;
        r.n_image = r.n_total = (double)n;
        r.slots = slots;
        r.l1_mean = l1_mean;
        loss_reduce_kernel<<<1, kBlock, 0, s>>>(r);
        r3::check_launch("loss reduce", s, false);
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

}  // extern "C"
