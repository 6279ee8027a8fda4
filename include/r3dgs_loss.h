/* r3dgs_loss.h -- C ABI of the fused training loss of train.py:109-115,
 *   loss = (1 - lambda) * L1(image, gt) + lambda * (1 - SSIM(image, gt)),
 * replacing utils/loss_utils.py:17-66 (l1_loss, ssim: five 11x11 depthwise convolutions, ~15 elementwise ops and
 * autograd's backward of all of them) by one forward launch pair and one backward launch (reduced-3dgs_amd/csrc/loss.hip).
 * Same conventions as r3dgs_rasterizer.h: device pointers, fp32, contiguous; `void* stream` is a hipStream_t; return >= 0
 * on success, < 0 with the message in r3dgs_last_error().  No call synchronises the host or allocates, so a forward +
 * backward pair can be captured in a graph.  No float atomics: values and gradients are identical run to run.
 *
 * Images are B x C planes of H x W (any B, C, H, W >= 1).  The window is the reference's: 11 taps, sigma 1.5, the fp32
 * weights of r3dgs_ssim_window, applied separably with zero padding 5.  Gradients are taken with respect to img1 only. */
#ifndef R3DGS_LOSS_H
#define R3DGS_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's 1-D window (utils/loss_utils.py:24-26): exp(-(i-5)^2 / 4.5) rounded to fp32, divided by their fp32 sum.
 * Host only; needs no GPU. */
void r3dgs_ssim_window(float w[11]);

/* Device scratch of r3dgs_l1_ssim_forward for this shape (per-workgroup partial sums; 0 for an invalid shape). */
size_t r3dgs_l1_ssim_workspace_bytes(int B, int C, int H, int W);

/* Forward: per pixel the SSIM value and |img1 - img2|, per workgroup their sums in fixed workspace slots, then one small
 * launch that adds the slots in a fixed order.  Every output pointer may be NULL (not written):
 *   l1_mean[1]      mean |img1 - img2| over all B*C*H*W elements
 *   ssim_mean[1]    mean SSIM over all elements
 *   ssim_image[B]   per-image mean SSIM (over C*H*W)
 *   loss[1]         (1 - lambda_dssim) * l1_mean + lambda_dssim * (1 - ssim_mean)
 *   dssim[1]        1 - ssim_mean
 *   ssim_map        [B,C,H,W] the SSIM map (aggregate=False)
 *   partials        [3,B,C,H,W] dS/dmu_x, dS/dE_xx, dS/dE_xy per pixel, for r3dgs_l1_ssim_backward (NULL: no-grad mode)
 * workspace: r3dgs_l1_ssim_workspace_bytes(B, C, H, W) bytes. */
int r3dgs_l1_ssim_forward(int B, int C, int H, int W, const float* img1, const float* img2, float lambda_dssim,
                          float* l1_mean, float* ssim_mean, float* ssim_image, float* loss, float* dssim, float* ssim_map,
                          float* partials, char* workspace, void* stream);

/* Backward: grad_img1[B,C,H,W] =
 *     coef_l1 * grad_l1[0] * sign(img1 - img2) / (B*C*H*W)                      (torch's sign(0) = 0; grad_l1 may be NULL)
 *   + sum over pixels q of gS(q) * dS(q)/dimg1                                   (grad_ssim may be NULL)
 * with the upstream gradient of the SSIM map gS(q) = coef_ssim * (ssim_grad_mode
 *   0: grad_ssim[0] / (B*C*H*W)       -- of the mean over all elements
 *   1: grad_ssim[b] / (C*H*W)         -- of the per-image means, b the image of q
 *   2: grad_ssim[q]                   -- of the map itself, [B,C,H,W]).
 * partials: what r3dgs_l1_ssim_forward wrote for the same img1, img2.  All upstream gradients are device pointers. */
int r3dgs_l1_ssim_backward(int B, int C, int H, int W, const float* img1, const float* img2, const float* partials,
                           const float* grad_l1, float coef_l1, const float* grad_ssim, int ssim_grad_mode, float coef_ssim,
                           float* grad_img1, void* stream);

/* L1 alone on n elements of any shape (utils/loss_utils.py:17-18): l1_mean[1] = mean |x - y| (same fixed-order reduction);
 * workspace: r3dgs_l1_workspace_bytes(n) bytes.  Backward: grad_x[n] = grad[0] * sign(x - y) / n. */
size_t r3dgs_l1_workspace_bytes(long long n);
int r3dgs_l1_forward(long long n, const float* x, const float* y, float* l1_mean, char* workspace, void* stream);
int r3dgs_l1_backward(long long n, const float* x, const float* y, const float* grad, float* grad_x, void* stream);

/* ---- The same loss behind a per-image exposure and a pixel mask (the official 3DGS train.py of Oct 2024: a learnable 3 x 4
 * colour map per training image, `image *= alpha_mask`), fused into the tile kernels instead of a dozen torch passes in front:
 *   x'_c(p)  = sum_k E[k][c] * x_k(p) + E[c][3]        (the pixel as a row vector times E[:, :3], plus the last column)
 *   x''_c(p) = m(p) * x'_c(p)
 *   y'_c(p)  = mask_target ? m(p) * y_c(p) : y_c(p)
 *   loss     = (1 - lambda) * mean |x'' - y'| + lambda * (1 - mean SSIM(x'', y'))
 * The means run over all B*C*H*W elements (no renormalisation by the mask's area).
 *   exposure  [B][3][4] (exposure_per_image != 0) or one [3][4] shared by the batch, row-major; NULL: the identity.
 *             An exposure needs C == 3.
 *   mask      [B][H][W] (mask_per_image != 0) or one [H][W] shared by the batch; NULL: ones.  Any C with a mask alone.
 * With exposure == NULL and mask == NULL, or E = eye(3,4) and a mask of ones, every output and grad_img1 equal those of
 * r3dgs_l1_ssim_forward / _backward bit for bit.  Gradients are taken with respect to img1 and the exposure.
 *
 * workspace: r3dgs_exposure_loss_workspace_bytes(B, C, H, W) bytes (0 for an invalid shape), 8-byte aligned, the same buffer
 * or two different ones for the two calls; workspace_bytes is its size; a shorter or misaligned one is refused.  Nothing in it has to
 * survive between the calls and nothing has to be cleared. */
size_t r3dgs_exposure_loss_workspace_bytes(int B, int C, int H, int W);

/* Outputs as r3dgs_l1_ssim_forward's (each may be NULL); partials [3,B,C,H,W] are those of (x'', y') for
 * r3dgs_exposure_loss_backward (NULL: no-grad mode). */
int r3dgs_exposure_loss_forward(int B, int C, int H, int W, const float* img1, const float* img2, const float* exposure,
                                int exposure_per_image, const float* mask, int mask_per_image, int mask_target,
                                float lambda_dssim, float* l1_mean, float* ssim_mean, float* ssim_image, float* loss,
                                float* dssim, float* partials, char* workspace, size_t workspace_bytes, void* stream);

/* With g = dL/dx'' = coef_l1 * grad_loss[0] * sign(x'' - y') / n + coef_ssim * grad_loss[0] / n * sum_q dS(q)/dx''
 * (n = B*C*H*W; the loss itself: coef_l1 = 1 - lambda, coef_ssim = -lambda; grad_loss a device pointer):
 *   grad_img1[B,C,H,W]   dx_k = m * sum_c E[k][c] * g_c
 *   grad_exposure        [B][3][4], or [3][4] for a shared exposure (the sum over the images): dE[k][c] = sum_p m g_c x_k,
 *                        dE[c][3] = sum_p m g_c; double sums in a fixed order, rounded to fp32 once.  NULL: not wanted.
 * The same img1, img2, exposure, mask and flags as the forward that wrote `partials`. */
int r3dgs_exposure_loss_backward(int B, int C, int H, int W, const float* img1, const float* img2, const float* exposure,
                                 int exposure_per_image, const float* mask, int mask_per_image, int mask_target,
                                 const float* partials, const float* grad_loss, float coef_l1, float coef_ssim,
                                 float* grad_img1, float* grad_exposure, char* workspace, size_t workspace_bytes, void* stream);

/* out[B,3,H,W] = x E[:, :3] + E[:, 3] per pixel, clamped to [0, 1] when clamp01 != 0: the exposed image for evaluation and
 * saving (train_test_exp).  No gradient.  out must not overlap img. */
int r3dgs_exposure_apply(int B, int H, int W, const float* img, const float* exposure, int exposure_per_image, int clamp01,
                         float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_LOSS_H */
