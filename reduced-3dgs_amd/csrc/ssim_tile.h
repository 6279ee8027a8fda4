// ssim_tile.h -- the tiled 11x11 window filter and the fixed-order sums shared by loss.hip (ssim_fwd_kernel, ssim_bwd_kernel)
// and metrics.hip (image_metrics_kernel), so that the SSIM evaluation reports is the SSIM the training loss sees.
//
// One 256-thread workgroup takes one 64 x 16 output tile of one plane.  M maps are staged with their 5-pixel halo in LDS
// (zeros outside the image: the reference's zero padding), filtered horizontally into LDS and vertically in registers
// (separable window, the reference's fp32 1-D weights); each thread ends with the M filtered values of kRows consecutive
// rows of one column.  Tile shape, padding rule and tap order are stated here and nowhere else.  Header-only and inlined:
// each unit compiles it under its own flags (build.py: loss.hip with contraction, metrics.hip without).
// No atomics anywhere: every sum has a fixed order.
#ifndef R3DGS_SSIM_TILE_H
#define R3DGS_SSIM_TILE_H

#include <hip/hip_runtime.h>

#include <cmath>

#include "loss_math.h"

namespace r3 {

constexpr int kBlock = 256;
constexpr int kTW = 64;                     // tile width: one wave spans a tile row
constexpr int kTH = 16;                     // tile height
constexpr int kRows = kTH / (kBlock / kTW); // output rows per thread (4)
constexpr int kInW = kTW + 2 * kSsimRadius; // staged width with halo (74)
constexpr int kInH = kTH + 2 * kSsimRadius; // staged height with halo (26)

struct Window {
    float w[kSsimTaps];
};

// utils/loss_utils.py:24-26: torch.Tensor([exp(...)]) rounds each double to fp32; gauss.sum() of the 11 fp32 values
// rounds to the same fp32 as their exact sum (checked bit for bit against the reference in tests/test_loss_cpu.py)
inline Window make_window()
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

inline const Window& window()
{
    static const Window w = make_window();
    return w;
}

struct Plane {
    int H, W, tiles_x, tiles_per_plane;
};

// workgroups of a tile kernel over `planes` planes of H x W, or -1 where there is nothing to do or 2^31 of them and more
inline long long tile_blocks(long long planes, int H, int W)
{
    if (planes < 1 || H < 1 || W < 1) return -1;
    const long long tiles = ((W + kTW - 1LL) / kTW) * ((H + kTH - 1LL) / kTH);
    return tiles > 0x7fffffffLL / planes ? -1 : planes * tiles;
}

// of a shape tile_blocks accepts
inline Plane plane_of(int H, int W)
{
    Plane p;
    p.H = H;
    p.W = W;
    p.tiles_x = (int)((W + kTW - 1LL) / kTW);
    p.tiles_per_plane = (int)tile_blocks(1, H, W);
    return p;
}

// the workgroup's plane and the image coordinates of its tile's first output pixel
struct Tile {
    int plane, gx0, gy0;
};

__device__ __forceinline__ Tile tile_of(const Plane& p)
{
    const int plane = blockIdx.x / p.tiles_per_plane, tile = blockIdx.x - plane * p.tiles_per_plane;
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    return Tile{plane, tx * kTW, ty * kTH};
}

// Fills the M staged tiles: load(gy, gx, v) gives the M values of an in-image pixel, everything else is zero.
template <int M, class Load>
__device__ __forceinline__ void stage_tiles(const Plane& p, const Tile& tl, float (&st)[M][kInH][kInW], Load load)
{
    for (int e = threadIdx.x; e < kInH * kInW; e += kBlock) {
        const int r = e / kInW, c = e - r * kInW;
        const int gy = tl.gy0 - kSsimRadius + r, gx = tl.gx0 - kSsimRadius + c;
        float v[M];
#pragma unroll
        for (int m = 0; m < M; m++) v[m] = 0.f;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) load(gy, gx, v);
#pragma unroll
        for (int m = 0; m < M; m++) st[m][r][c] = v[m];
    }
    __syncthreads();
}

// The taps of the forward kernels: x, y, x*x, y*y, x*y from the staged pair (x, y).
struct MomentTaps {
    const float (&st)[2][kInH][kInW];
    __device__ __forceinline__ void operator()(int r, int c, float (&v)[5]) const
    {
        const float xv = st[0][r][c], yv = st[1][r][c];
        v[0] = xv;
        v[1] = yv;
        v[2] = xv * xv;
        v[3] = yv * yv;
        v[4] = xv * yv;
    }
};

// The separable filter of M maps: taps(r, c, v) gives the M values at staged position (r, c).  On return acc[o][m] is map m
// filtered at this thread's output pixel o (for_each_output); `sh` is the workgroup's scratch between the passes.
template <int M, class Taps>
__device__ __forceinline__ void filter_tile(const Window& win, float (&sh)[M][kInH][kTW], float (&acc)[kRows][M], Taps taps)
{
    const int c = threadIdx.x & (kTW - 1), rg = threadIdx.x / kTW;
    // horizontal pass: (kInH rows) x (kTW columns)
    for (int r = rg; r < kInH; r += kBlock / kTW) {
        float h[M];
#pragma unroll
        for (int m = 0; m < M; m++) h[m] = 0.f;
#pragma unroll
        for (int k = 0; k < kSsimTaps; k++) {
            const float w = win.w[k];
            float v[M];
            taps(r, c + k, v);
#pragma unroll
            for (int m = 0; m < M; m++) h[m] = fmaf(w, v[m], h[m]);
        }
#pragma unroll
        for (int m = 0; m < M; m++) sh[m][r][c] = h[m];
    }
    __syncthreads();
    // vertical pass: this thread's kRows consecutive output rows of column c
    const int r0 = rg * kRows;
#pragma unroll
    for (int o = 0; o < kRows; o++)
#pragma unroll
        for (int m = 0; m < M; m++) acc[o][m] = 0.f;
#pragma unroll
    for (int j = 0; j < kRows + 2 * kSsimRadius; j++) {
        float v[M];
#pragma unroll
        for (int m = 0; m < M; m++) v[m] = sh[m][r0 + j][c];
#pragma unroll
        for (int o = 0; o < kRows; o++) {
            const int k = j - o;
            if (k >= 0 && k < kSsimTaps) {
#pragma unroll
                for (int m = 0; m < M; m++) acc[o][m] = fmaf(win.w[k], v[m], acc[o][m]);
            }
        }
    }
}

// f(o, gy, gx, r, c) for each of this thread's kRows output pixels that lie inside the image: o indexes acc, (gy, gx) is
// the pixel, (r, c) its place in the staged tiles.
template <class F>
__device__ __forceinline__ void for_each_output(const Plane& p, const Tile& tl, F f)
{
    const int c = threadIdx.x & (kTW - 1), r0 = threadIdx.x / kTW * kRows;
    const int gx = tl.gx0 + c;
#pragma unroll
    for (int o = 0; o < kRows; o++) {
        const int gy = tl.gy0 + r0 + o;
        if (gx >= p.W || gy >= p.H) continue;
        f(o, gy, gx, r0 + o + kSsimRadius, c + kSsimRadius);
    }
}

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// N block-wide sums in a fixed order; thread 0 gets the results.
template <class T, int N>
__device__ __forceinline__ void block_sums(T (&v)[N], T (*red)[kBlock / 64])
{
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        v[k] = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    }
}

// kBlock-wide tree sum of v in a fixed order through `buf`; every thread gets the total.
template <class T>
__device__ __forceinline__ T tree_sum(T v, T* buf)
{
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
        if (t < stride) buf[t] += buf[t + stride];
        __syncthreads();
    }
    const T total = buf[0];
    __syncthreads();
    return total;
}

// The finishing sums of N runs of `count` per-workgroup slots: one thread-strided loop adds all N in double, then each goes
// through the fixed tree in its own row of `buf`; every thread gets the totals.
template <int N, class T>
__device__ __forceinline__ void slot_sums(const T* const (&run)[N], int count, double (&sum)[N], double (&buf)[N][kBlock])
{
#pragma unroll
    for (int k = 0; k < N; k++) sum[k] = 0.0;
    for (int i = threadIdx.x; i < count; i += kBlock) {
#pragma unroll
        for (int k = 0; k < N; k++) sum[k] += run[k][i];
    }
#pragma unroll
    for (int k = 0; k < N; k++) sum[k] = tree_sum(sum[k], buf[k]);
}

}  // namespace r3

#endif  // R3DGS_SSIM_TILE_H
