/* r3dgs_trainstats.h -- C ABI of the per-iteration training statistics: the visibility-masked bookkeeping the reference's
 * loop runs around loss.backward(), without boolean-mask indexing (every `x[mask]` of the reference runs `nonzero`, which
 * blocks the host until the stream has drained).  Same conventions as r3dgs_rasterizer.h / r3dgs_reduction.h: device
 * pointers, fp32 / int32, contiguous; `void* stream` is a hipStream_t; return >= 0 on success, < 0 with the message in
 * r3dgs_last_error().  Every call is enqueued on the caller's stream, synchronises nothing, allocates nothing and can be
 * captured in a graph (the launches of one call form a chain).  P <= 0 is a no-op returning 0.
 *
 * Lines of the reference each entry point replaces, with vis_i = radii[i] > 0 (render()'s visibility_filter):
 *   r3dgs_visible_means         train.py:105-106  Lalpha_regul = gaussians.get_opacity[visibility_filter].abs().mean()
 *                               train.py:113      gaussians._features_rest.detach()[visibility_filter].abs().mean()
 *   r3dgs_alpha_regul_backward  the autograd backward of train.py:105-106 (index, sigmoid)
 *   r3dgs_densification_stats   train.py:134      max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis])
 *                               scene/gaussian_model.py:693-695  xyz_gradient_accum += norm(viewspace.grad[:, :2]); denom += vis
 */
#ifndef R3DGS_TRAINSTATS_H
#define R3DGS_TRAINSTATS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch r3dgs_visible_means needs for P Gaussians (its per-workgroup partial sums); 0 for P <= 0.
 * A pure function of P: no device is touched. */
size_t r3dgs_train_stats_workspace_bytes(int P);

/* The two visibility-masked means of train.py:105-106 and :113, the visible count and the mask, in two chained launches:
 *   visibility[i] = radii[i] > 0                                   uint8 [P], 0 / 1
 *   n_visible     = sum_i visibility[i]                            int32
 *   alpha_mean    = sum_vis sigmoid(opacity[i]) / n_visible        sigmoid(x) = 1 / (1 + exp(-x)): opacity is the RAW parameter
 *   sh_abs_mean   = sum_vis sum_row |features_rest[i]| / (n_visible * 3 (M - 1))
 * radii: int32 [P].  alpha_mean may be NULL (not wanted), else opacity: fp32 [P] is required.  sh_abs_mean may be NULL (not
 * wanted), else features_rest: fp32 [P, M-1, 3] is required when M > 1; M >= 1 is the coefficient count INCLUDING the DC
 * term, as the rasterizer counts it.  Only 16-byte words of features_rest that overlap a visible Gaussian's row are loaded.
 * Empty means follow torch: n_visible == 0 gives NaN for both; M == 1 (no rest coefficients) gives sh_abs_mean = NaN.
 * Sums are accumulated in double per lane, wave and workgroup; the second launch adds the workgroups' partial sums in a
 * fixed order, so the three numbers are bit-identical from run to run for the same inputs (no atomics).
 * workspace: r3dgs_train_stats_workspace_bytes(P) bytes, 8-byte aligned; it need not be cleared. */
int r3dgs_visible_means(int P, int M, const int* radii, const float* opacity, const float* features_rest,
                        uint8_t* visibility, int* n_visible, float* alpha_mean, float* sh_abs_mean, char* workspace,
                        void* stream);

/* Backward of alpha_mean with respect to the raw opacity (autograd of train.py:105-106), one elementwise launch:
 *   dL_dopacity[i] += upstream[0] * vis_i * s_i (1 - s_i) / n_visible[0],    s_i = sigmoid(opacity[i])
 * upstream: device fp32 scalar (the autograd gradient of alpha_mean; never read by the host); n_visible: the device
 * int32 r3dgs_visible_means left.  It ADDS into dL_dopacity [P]; rows of culled Gaussians are not touched, and with
 * n_visible == 0 nothing is. */
int r3dgs_alpha_regul_backward(int P, const int* radii, const float* opacity, const float* upstream, const int* n_visible,
                               float* dL_dopacity, void* stream);

/* The densification statistics of one iteration (train.py:134, scene/gaussian_model.py:693-695), one launch, in place:
 *   xyz_gradient_accum[i] += vis_i ? sqrtf(gx * gx + gy * gy) : 0      (gx, gy) = viewspace_grad[i, 0:2]
 *   denom[i]              += vis_i ? 1 : 0
 *   max_radii2D[i]         = vis_i ? max(max_radii2D[i], (float)radii[i]) : max_radii2D[i]
 * viewspace_grad: fp32 [P,3] (gradient of the means2D dummy); xyz_gradient_accum, denom: fp32 [P,1]; max_radii2D: fp32
 * [P], as the reference stores them.  The reference adds the norm of EVERY row; the backward writes all-zero rows for
 * culled Gaussians, so the two definitions agree -- here a culled Gaussian's row is not even read. */
int r3dgs_densification_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum, float* denom,
                              float* max_radii2D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_TRAINSTATS_H */
