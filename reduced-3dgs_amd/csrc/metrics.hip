// metrics.hip -- the evaluation metrics (include/r3dgs_metrics.h): L1, MSE, PSNR and SSIM of a view against its ground truth.
//
// What the reference does (train.py:253-265; render.py + metrics.py:24-86): two clamps, l1_loss, psnr and, for metrics.py,
// the torch-formula ssim -- five 11x11 depthwise convolutions and ~15 full-size intermediate maps -- per view, and one
// .item()-style host read per metric per view.  How it is issued here:
//   * image_metrics_kernel: one workgroup per tile of one channel plane, on the tile filter of ssim_tile.h that loss.hip's
//     ssim_fwd_kernel runs on.  Image and ground truth are staged ONCE through metrics_math.h's metrics_load (uint8 truth,
//     either layout, clamp, 8-bit rounding of the render); their five moments are filtered and loss_math.h gives S per
//     pixel.  |x - y| and (x - y)^2 are taken in double from the staged values.  The workgroup writes its three double sums
//     to its own workspace slots.  Nothing else is stored: no map, no partials for a backward.
//   * metrics_finish_kernel: one workgroup adds the slots channel by channel in a fixed order and writes the row.
//   * row_mse_kernel (+ row_mse_finish_kernel for rows longer than one chunk): the drop-in mse / psnr of any [R, n] view.
//   * to_uint8_kernel: CHW float -> HWC bytes through metrics_quantise8.
// No atomics anywhere: every sum has a fixed order (ssim_tile.h), so results are identical run to run.
#include "../../include/r3dgs_metrics.h"

#include "common.h"
#include "loss_math.h"
#include "metrics_math.h"
#include "ssim_tile.h"

using namespace r3;

namespace {

constexpr int kSums = 3;                    // per-workgroup slots: sum |x - y|, sum (x - y)^2, sum S
constexpr int kMseChunk = 16 * kBlock;      // elements per workgroup of row_mse_kernel

struct MetricsArgs {
    int C;
    Plane p;
    int flags;
    const float* x;
    const void* y;
    double* slots;   // [C * tiles_per_plane][kSums]
    Window win;
};

template <int Layout>
__device__ __forceinline__ float load_gt(const void* y, int C, int H, int W, int c, int gy, int gx, int flags)
{
    const size_t pix = (size_t)gy * W + gx;
    if (Layout == R3DGS_GT_F32_CHW)
        return r3::metrics_load(static_cast<const float*>(y)[(size_t)c * H * W + pix], flags & r3::kMetricsClamp);
    if (Layout == R3DGS_GT_U8_CHW) return r3::metrics_load(static_cast<const uint8_t*>(y)[(size_t)c * H * W + pix], 0);
    return r3::metrics_load(static_cast<const uint8_t*>(y)[pix * C + c], 0);
}

template <int Layout>
__global__ __launch_bounds__(kBlock) void image_metrics_kernel(MetricsArgs a)
{
    __shared__ float sxy[2][kInH][kInW];
    __shared__ float sh[5][kInH][kTW];
    __shared__ double red[kSums][kBlock / 64];
    const int H = a.p.H, W = a.p.W;
    const Tile tl = tile_of(a.p);
    const float* X = a.x + (size_t)tl.plane * H * W;
    stage_tiles(a.p, tl, sxy, [&](int gy, int gx, float (&v)[2]) {
        v[0] = metrics_load(X[(size_t)gy * W + gx], a.flags);
        v[1] = load_gt<Layout>(a.y, a.C, H, W, tl.plane, gy, gx, a.flags);
    });
    float acc[kRows][5];
    filter_tile(a.win, sh, acc, MomentTaps{sxy});
    double sums[kSums] = {0.0, 0.0, 0.0};
    for_each_output(a.p, tl, [&](int o, int, int, int r, int c) {
        const float xv = sxy[0][r][c], yv = sxy[1][r][c];
        sums[0] += metrics_abs_err(xv, yv);
        sums[1] += metrics_sq_err(xv, yv);
        sums[2] += (double)ssim_pixel(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4]).s;
    });
    block_sums(sums, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; k++) a.slots[(size_t)blockIdx.x * kSums + k] = sums[k];
    }
}

__host__ __device__ inline double psnr_db(double mse) { return 10.0 * log10(1.0 / mse); }

// One workgroup: per channel, thread-strided double sums of its tiles' slots and a fixed tree; channels in order.
__global__ __launch_bounds__(kBlock) void metrics_finish_kernel(int C, int tiles_per_plane, double n_plane,
                                                                const double* __restrict__ slots, double* __restrict__ row)
{
    __shared__ double buf[kBlock];
    const int t = threadIdx.x;
    double tot[kSums] = {0.0, 0.0, 0.0}, mse_c[4] = {0.0, 0.0, 0.0, 0.0}, psnr_c = 0.0;
    for (int c = 0; c < C; c++) {
        double s[kSums] = {0.0, 0.0, 0.0};
        const double* first = slots + (size_t)c * tiles_per_plane * kSums;
        for (int i = t; i < tiles_per_plane; i += kBlock) {
#pragma unroll
            for (int k = 0; k < kSums; k++) s[k] += first[(size_t)i * kSums + k];
        }
#pragma unroll
        for (int k = 0; k < kSums; k++) {
            s[k] = tree_sum(s[k], buf);
            tot[k] += s[k];
        }
        mse_c[c] = s[1] / n_plane;
        psnr_c += psnr_db(mse_c[c]);
    }
    if (t == 0) {
        const double n = n_plane * (double)C, mse = tot[1] / n;
        row[R3DGS_METRICS_L1] = tot[0] / n;
        row[R3DGS_METRICS_MSE] = mse;
        for (int c = 0; c < 4; c++) row[R3DGS_METRICS_MSE_C + c] = mse_c[c];
        row[R3DGS_METRICS_PSNR_IMAGE] = psnr_db(mse);
        row[R3DGS_METRICS_PSNR_CHANNELS] = psnr_c / (double)C;
        row[R3DGS_METRICS_SSIM] = tot[2] / n;
    }
}

// Workgroup b takes chunk b % chunks of row b / chunks: 16 elements per thread, double sums in a fixed order.  A row of one
// chunk is finished here (mean into mse[row]); longer rows leave their chunk sums in slots[b] for row_mse_finish_kernel.
__global__ __launch_bounds__(kBlock) void row_mse_kernel(long long n, long long chunks, const float* __restrict__ a,
                                                         const float* __restrict__ b, double* __restrict__ slots,
                                                         double* __restrict__ mse)
{
    __shared__ double red[1][kBlock / 64];
    const long long row = (long long)blockIdx.x / chunks, chunk = (long long)blockIdx.x - row * chunks;
    const float* pa = a + (size_t)row * (size_t)n;
    const float* pb = b + (size_t)row * (size_t)n;
    double s[1] = {0.0};
#pragma unroll
    for (int i = 0; i < kMseChunk / kBlock; i++) {
        const long long e = chunk * kMseChunk + i * kBlock + threadIdx.x;
        if (e < n) s[0] += r3::metrics_sq_err(pa[e], pb[e]);
    }
    block_sums(s, red);
    if (threadIdx.x == 0) {
        if (chunks == 1)
            mse[row] = s[0] / (double)n;
        else
            slots[blockIdx.x] = s[0];
    }
}

// One workgroup per row: thread-strided double sums of the row's chunk slots and a fixed tree.
__global__ __launch_bounds__(kBlock) void row_mse_finish_kernel(long long n, long long chunks, const double* __restrict__ slots,
                                                                double* __restrict__ mse)
{
    __shared__ double buf[kBlock];
    const double* first = slots + (size_t)blockIdx.x * (size_t)chunks;
    double s = 0.0;
    for (long long i = threadIdx.x; i < chunks; i += kBlock) s += first[i];
    s = tree_sum(s, buf);
    if (threadIdx.x == 0) mse[blockIdx.x] = s / (double)n;
}

// out[(y * W + x) * C + c] = quantise8(image[c][y][x]): consecutive threads write consecutive bytes
__global__ __launch_bounds__(kBlock) void to_uint8_kernel(int C, long long plane, const float* __restrict__ image,
                                                          unsigned char* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= plane * C) return;
    const long long pix = e / C;
    const int c = (int)(e - pix * C);
    out[e] = r3::metrics_quantise8(image[(size_t)c * plane + pix]);
}

// workgroups of image_metrics_kernel, or -1 for a shape the entry points refuse
long long metrics_blocks(int C, int H, int W)
{
    return C < 1 || C > 4 ? -1 : tile_blocks(C, H, W);
}

long long mse_chunks(long long R, long long n)
{
    if (R < 1 || n < 1) return -1;
    const long long chunks = (n + kMseChunk - 1) / kMseChunk;
    return chunks > 0x7fffffffLL / R ? -1 : chunks;   // R * chunks workgroups in one grid
}

}  // namespace

extern "C" {

size_t r3dgs_image_metrics_workspace_bytes(int C, int H, int W)
{
    const long long nb = metrics_blocks(C, H, W);
    return nb < 0 ? 0 : (size_t)nb * kSums * sizeof(double);
}

int r3dgs_image_metrics(int C, int H, int W, const float* image, const void* gt, int gt_layout, int flags, double* row,
                        char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        const long long nb = metrics_blocks(C, H, W);
        if (nb < 0)
            throw r3::Error("image_metrics: need 1 <= C <= 4, H, W >= 1 and fewer than 2^31 tiles, got " + std::to_string(C) +
                            "x" + std::to_string(H) + "x" + std::to_string(W));
        if (gt_layout != R3DGS_GT_F32_CHW && gt_layout != R3DGS_GT_U8_CHW && gt_layout != R3DGS_GT_U8_HWC)
            throw r3::Error("image_metrics: unknown ground-truth layout " + std::to_string(gt_layout));
        if (flags & ~(R3DGS_METRICS_CLAMP | R3DGS_METRICS_QUANTISE8))
            throw r3::Error("image_metrics: unknown flag bits in " + std::to_string(flags));
        if (!image || !gt || !row || !workspace) throw r3::Error("image_metrics: a required pointer is NULL");
        if (reinterpret_cast<uintptr_t>(workspace) % alignof(double) || reinterpret_cast<uintptr_t>(row) % alignof(double))
            throw r3::Error("image_metrics: row and workspace must be 8-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        MetricsArgs a;
        a.C = C;
        a.p = plane_of(H, W);
        a.flags = flags;
        a.x = image;
        a.y = gt;
        a.slots = reinterpret_cast<double*>(workspace);
        a.win = window();
        if (gt_layout == R3DGS_GT_F32_CHW)
            image_metrics_kernel<R3DGS_GT_F32_CHW><<<(int)nb, kBlock, 0, s>>>(a);
        else if (gt_layout == R3DGS_GT_U8_CHW)
            image_metrics_kernel<R3DGS_GT_U8_CHW><<<(int)nb, kBlock, 0, s>>>(a);
        else
            image_metrics_kernel<R3DGS_GT_U8_HWC><<<(int)nb, kBlock, 0, s>>>(a);
        r3::check_launch("image metrics", s, false);
        metrics_finish_kernel<<<1, kBlock, 0, s>>>(C, a.p.tiles_per_plane, (double)H * (double)W, a.slots, row);
        r3::check_launch("metrics finish", s, false);
        return 0;
    });
}

size_t r3dgs_row_mse_workspace_bytes(long long R, long long n)
{
    const long long chunks = mse_chunks(R, n);
    return chunks < 0 ? 0 : (size_t)(R * chunks) * sizeof(double);
}

int r3dgs_row_mse(long long R, long long n, const float* a, const float* b, double* mse, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        const long long chunks = mse_chunks(R, n);
        if (chunks < 0)
            throw r3::Error("row_mse: need R, n >= 1 and fewer than 2^31 chunks of " + std::to_string(kMseChunk) +
                            " elements, got " + std::to_string(R) + " rows of " + std::to_string(n));
        if (!a || !b || !mse || !workspace) throw r3::Error("row_mse: a required pointer is NULL");
        if (reinterpret_cast<uintptr_t>(workspace) % alignof(double) || reinterpret_cast<uintptr_t>(mse) % alignof(double))
            throw r3::Error("row_mse: mse and workspace must be 8-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        double* slots = reinterpret_cast<double*>(workspace);
        row_mse_kernel<<<(int)(R * chunks), kBlock, 0, s>>>(n, chunks, a, b, slots, mse);
        r3::check_launch("row mse", s, false);
        if (chunks > 1) {
            row_mse_finish_kernel<<<(int)R, kBlock, 0, s>>>(n, chunks, slots, mse);
            r3::check_launch("row mse finish", s, false);
        }
        return 0;
    });
}

int r3dgs_image_to_uint8(int C, int H, int W, const float* image, unsigned char* out_hwc, void* stream)
{
    return r3::guarded_call([&]() {
        const long long plane = (H < 1 || W < 1) ? -1 : (long long)H * W;
        const long long total = (C < 1 || C > 4 || plane < 0 || plane > (1LL << 39)) ? -1 : plane * C;
        if (total < 0 || (total + kBlock - 1) / kBlock > 0x7fffffffLL)
            throw r3::Error("image_to_uint8: need 1 <= C <= 4, H, W >= 1 and fewer than 2^39 elements, got " +
                            std::to_string(C) + "x" + std::to_string(H) + "x" + std::to_string(W));
        if (!image || !out_hwc) throw r3::Error("image_to_uint8: a required pointer is NULL");
        hipStream_t s = static_cast<hipStream_t>(stream);
        to_uint8_kernel<<<(int)((total + kBlock - 1) / kBlock), kBlock, 0, s>>>(C, plane, image, out_hwc);
        r3::check_launch("image to uint8", s, false);
        return 0;
    });
}

}  // extern "C"
