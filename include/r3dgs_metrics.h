/* r3dgs_metrics.h -- C ABI of the evaluation metrics: L1, MSE, PSNR and SSIM of a rendered view against its ground truth,
 * the numbers the reference judges a model by (train.py:246-269 training_report; render.py followed by metrics.py:71-86),
 * in one fused pass per view (reduced-3dgs_amd/csrc/metrics.hip).  LPIPS is not covered.
 * Same conventions as r3dgs_loss.h: device pointers, contiguous; `void* stream` is a hipStream_t; return >= 0 on success,
 * < 0 with the message in r3dgs_last_error().  No call synchronises the host or allocates, so the calls can be captured in a
 * graph (each is a chain of launches on `stream`).  No float atomics: results are identical run to run. */
#ifndef R3DGS_METRICS_H
#define R3DGS_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout of the ground truth handed to r3dgs_image_metrics. */
#define R3DGS_GT_F32_CHW 0 /* float [C,H,W] */
#define R3DGS_GT_U8_CHW 1  /* unsigned char [C,H,W]; a sample u is compared as float(u) / 255.0f (to_tensor) */
#define R3DGS_GT_U8_HWC 2  /* unsigned char [H,W,C], what an image decoder hands over */

/* Flag bits of r3dgs_image_metrics.  Both apply to the image; CLAMP also applies to a float ground truth.
 *   CLAMP      min(max(x, 0), 1) before the comparison (train.py:256-257); NaN stays NaN
 *   QUANTISE8  the image is rounded to 8 bits the way save_image rounds it -- mul(255), add(0.5), clamp(0, 255), truncate,
 *              each step in fp32 -- and compared as that byte / 255.0f: what metrics.py reads back from the PNG render.py
 *              wrote.  NaN becomes 0 (the reference leaves that case undefined). */
#define R3DGS_METRICS_CLAMP 1
#define R3DGS_METRICS_QUANTISE8 2

/* One result row: R3DGS_METRICS_ROW doubles.  Entries that do not apply (mse_c of channels >= C) are 0.
 *   [L1]             mean |x - y| over all C*H*W elements
 *   [MSE]            mean (x - y)^2 over all elements
 *   [MSE_C + c]      mean (x - y)^2 over channel c, c < 4
 *   [PSNR_IMAGE]     10 log10(1 / mse): metrics.py:73, psnr of a [1,C,H,W] batch (one mean over the image)
 *   [PSNR_CHANNELS]  mean over channels of 10 log10(1 / mse_c): train.py:263, psnr(image [C,H,W]).mean()
 *   [SSIM]           mean over all elements of the SSIM map (11-tap window of r3dgs_ssim_window, zero padding 5, over the
 *                    loaded values)
 * A zero mse gives +inf; NaN propagates. */
#define R3DGS_METRICS_ROW 9
#define R3DGS_METRICS_L1 0
#define R3DGS_METRICS_MSE 1
#define R3DGS_METRICS_MSE_C 2
#define R3DGS_METRICS_PSNR_IMAGE 6
#define R3DGS_METRICS_PSNR_CHANNELS 7
#define R3DGS_METRICS_SSIM 8

/* Device scratch of r3dgs_image_metrics for this shape (per-workgroup partial sums; 0 for an invalid shape). */
size_t r3dgs_image_metrics_workspace_bytes(int C, int H, int W);

/* image: float [C,H,W], 1 <= C <= 4.  gt: as gt_layout says.  row: R3DGS_METRICS_ROW doubles on the device.
 * One tile kernel (partial sums in fixed workspace slots) and one one-workgroup launch that adds them in a fixed order. */
int r3dgs_image_metrics(int C, int H, int W, const float* image, const void* gt, int gt_layout, int flags, double* row,
                        char* workspace, void* stream);

/* Mean squared error of R rows of n contiguous floats (utils/image_utils.py:14-15 with R = shape[0]): mse[R] doubles,
 * double sums in a fixed order.  Any R, n >= 1 (fewer than 2^31 workgroups of 4096 elements). */
size_t r3dgs_row_mse_workspace_bytes(long long R, long long n);
int r3dgs_row_mse(long long R, long long n, const float* a, const float* b, double* mse, char* workspace, void* stream);

/* save_image's conversion without the host: out_hwc[H,W,C] = the QUANTISE8 rounding of image[C,H,W]. */
int r3dgs_image_to_uint8(int C, int H, int W, const float* image, unsigned char* out_hwc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_METRICS_H */
