/* r3dgs_mip.h -- C ABI of the anti-aliasing unit: the per-view 2D opacity compensation and the 3D smoothing filter, as
 * differentiable maps from raw parameters to raw parameters that sit IN FRONT of the unchanged rasterizer (every forward
 * applies sigmoid to the raw opacity it is given, so a compensated opacity travels as its logit).  Same conventions as the
 * other units: device pointers, fp32, contiguous; `void* stream` is a hipStream_t; return 0 on success, < 0 with the message
 * in r3dgs_last_error(); P == 0 is valid and launches nothing.  Nothing here allocates, waits on the host or uses a float
 * atomic: every output is a function of the inputs alone, bit-identical from run to run, and every call is capturable in a
 * graph.  The per-Gaussian arithmetic is csrc/mip_math.h.
 *
 * 2D compensation (per view).  (a, b, c): the 2D covariance of the Gaussian BEFORE the forward's 0.3 dilation (the forward's
 * own expressions, 1.3 tan(fov) clamp and scale_modifier included);
 *   rho = sqrt(max(0.000025, (a c - b^2) / ((a + 0.3)(c + 0.3) - b^2)))     p = sigmoid(o) rho     raw_eff = log(p) - log1p(-p)
 * These are the `antialiasing` semantics of the official 3DGS rasterizer and gsplat's rasterize_mode="antialiased" with
 * eps2d = 0.3.  They are NOT Mip-Splatting's 2D filter (a 0.1 kernel in place of the dilation).  A Gaussian every forward culls
 * (view-space z <= 0.2) keeps raw_eff = o (rho = 1) and passes its gradient to o alone.  Below the 0.000025 floor rho is a
 * constant.  1 - p is floored at 2^-24.
 *
 * 3D smoothing filter (Mip-Splatting, per model).  A camera is valid for a Gaussian if its view-space z > 0.2 and
 * -0.15 W <= x / z focal_x + W / 2 <= 1.15 W, likewise in y.  d_i: the smallest z over the valid cameras; a Gaussian valid in no
 * camera takes the largest d of those that are (0 if none is);  filter_i = d_i / max_v focal_x * sqrt(0.2).  Applied:
 *   log_scale_eff_k = 0.5 log(exp(2 ls_k) + f^2)     coef = sqrt(prod_k s_k^2 / prod_k (s_k^2 + f^2))
 *   raw_eff = logit(sigmoid(o) coef)                 f == 0: the inputs, bit for bit.  f carries no gradient.
 */
#ifndef R3DGS_MIP_H
#define R3DGS_MIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3DGS_MIP_CAMERA_FLOATS 20 /* a row of the camera table: world_view_transform (16), focal_x, focal_y, W, H */

/* means3D [P,3]; opacities [P,1] raw; viewmatrix [16] on the device.  The covariance comes from cov3D_precomp [P,6] if it is
 * not NULL, else from scales [P,3] and rotations [P,4] (16-byte aligned): activated values (raw == 0), or the model's
 * _scaling / _rotation, activated by the kernel as the raw-parameter forward does (raw != 0; cov3D_precomp must be NULL).
 * raw_eff [P,1]; rho [P] or NULL. */
int r3dgs_mip_opacity(int P, const float* means3D, const float* scales, const float* rotations, const float* cov3D_precomp,
                      const float* opacities, int raw, const float* viewmatrix, float tan_fovx, float tan_fovy, int W, int H,
                      float scale_modifier, float* raw_eff, float* rho, void* stream);

/* The same inputs, and dL_draw_eff [P,1].  Outputs (any may be NULL; each one given is overwritten, every row written):
 * dL_dopacities [P,1], dL_dmeans3D [P,3], dL_dscales [P,3] and dL_drotations [P,4] (w.r.t. what was handed in: the raw
 * tensors if raw != 0; zero if cov3D_precomp is given), dL_dcov3D [P,6] (zero unless cov3D_precomp is given). */
int r3dgs_mip_opacity_backward(int P, const float* means3D, const float* scales, const float* rotations,
                               const float* cov3D_precomp, const float* opacities, int raw, const float* viewmatrix,
                               float tan_fovx, float tan_fovy, int W, int H, float scale_modifier, const float* dL_draw_eff,
                               float* dL_dopacities, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                               float* dL_dcov3D, void* stream);

/* Bytes of device scratch r3dgs_mip_filter3d needs; 0 for P <= 0.  A pure function of its arguments. */
size_t r3dgs_mip_filter3d_workspace_bytes(int P, int V);

/* means3D [P,3]; cameras [V, R3DGS_MIP_CAMERA_FLOATS] on the device; filter [P,1]; workspace: 16-byte aligned, not cleared.
 * Two launches: one lane per Gaussian loops over the cameras (staged through LDS in chunks), one workgroup takes the global
 * maximum (an integer maximum of the floats' bit patterns: exact, order-independent) and fills the rows no camera sees. */
int r3dgs_mip_filter3d(int P, int V, const float* means3D, const float* cameras, float* filter, char* workspace, void* stream);

/* scaling_raw [P,3] (log-scales), opacity_raw [P,1], filter [P,1] -> scaling_eff [P,3], opacity_eff [P,1].  One launch. */
int r3dgs_mip_filtered(int P, const float* scaling_raw, const float* opacity_raw, const float* filter, float* scaling_eff,
                       float* opacity_eff, void* stream);

/* dL_dscaling_eff [P,3], dL_dopacity_eff [P,1] (either may be NULL: zero) -> dL_dscaling_raw [P,3], dL_dopacity_raw [P,1]
 * (either may be NULL; overwritten). */
int r3dgs_mip_filtered_backward(int P, const float* scaling_raw, const float* opacity_raw, const float* filter,
                                const float* dL_dscaling_eff, const float* dL_dopacity_eff, float* dL_dscaling_raw,
                                float* dL_dopacity_raw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_MIP_H */
