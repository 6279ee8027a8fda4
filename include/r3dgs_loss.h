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

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_LOSS_H */
