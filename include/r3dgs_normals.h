/* r3dgs_normals.h -- C ABI of the surface-normal unit: the view-space normal of every Gaussian, the normal map derived from a
 * depth map by finite differences, and the depth-normal consistency loss L = mean w (1 - s N . n) of 2DGS / GOF / PGSR /
 * RaDe-GS, each forward and backward.  Same conventions as the other units: device pointers, fp32, contiguous; `void* stream`
 * is a hipStream_t; return 0 on success, < 0 with the message in r3dgs_last_error(); an empty problem (P == 0) is valid and
 * launches nothing.  Nothing here allocates, waits on the host or uses a float atomic: every output is a function of the
 * inputs alone, bit-identical from run to run, every call is capturable in a graph, and the loss and its upstream gradient
 * stay on the device.  The per-element arithmetic is csrc/normal_math.h.
 *
 * Normal of a Gaussian.  k: the index of the smallest of its three scales (the lowest index on a tie; raw log-scales have the
 * same argmin).  n_w: column k of R(q), the rotation of Sigma = R S^2 R^T that the rasterizer projects (the reference's
 * build_rotation), negated when n_w . (mean - campos) > 0 so that it faces the camera.  Result: n_w as a row vector times the
 * 3x3 block of the view matrix (how every kernel here takes a mean into the view frame).  The gradient reaches the quaternion
 * alone: the argmin and the sign are piecewise constant.
 *
 * Normal of a depth pixel.  z = depth / alpha where alpha >= R3DGS_NORMAL_ALPHA_MIN, else 0 (no alpha given: z = depth).
 * p(x, y) = z ((2 (x + 0.5) / W - 1) tan_fovx, (2 (y + 0.5) / H - 1) tan_fovy, 1): the pixel centres of the rasterizer.
 * d_v = p(x, y+1) - p(x, y-1), d_h = p(x+1, y) - p(x-1, y), c = d_v x d_h, n = c / |c|; n = 0 with a zero gradient when
 * |c|^2 <= R3DGS_NORMAL_CROSS_MIN, and on the one-pixel border.  A fronto-parallel plane gives (0, 0, -1).
 *
 * Loss.  L = 1 / (H W) sum_p w(p) (1 - s(p) N(p) . n(p)); N: the given (blended, unnormalised) normal map; s: alpha as a
 * CONSTANT (no gradient through this factor) if scale_by_alpha != 0 and alpha is given, else 1; w: pixel_weight or 1.  Double
 * sums in a fixed order, finished by one workgroup.
 */
#ifndef R3DGS_NORMALS_H
#define R3DGS_NORMALS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Below the smallest alpha of a pixel with one blended Gaussian (the blend skips alpha < 1/255): separates "nothing here". */
#define R3DGS_NORMAL_ALPHA_MIN 1e-3f
/* |c| <= 1e-12, the eps of the normalize in 2DGS's depth_to_normal. */
#define R3DGS_NORMAL_CROSS_MIN 1e-24f

/* means3D [P,3], scales [P,3], rotations [P,4], viewmatrix [16], campos [3] on the device -> normals [P,3].  raw == 0: the
 * rotations are used as given (unit quaternions); raw != 0: the model's _rotation, divided by max(|q|, 1e-12) in the kernel
 * (scales may then be the raw _scaling: the same argmin).  One launch. */
int r3dgs_gaussian_normals(int P, const float* means3D, const float* scales, const float* rotations, int raw,
                           const float* viewmatrix, const float* campos, float* normals, void* stream);

/* The same inputs and dL_dnormals [P,3] -> dL_drotations [P,4] (with respect to what was handed in; overwritten, every row
 * written).  One launch. */
int r3dgs_gaussian_normals_backward(int P, const float* means3D, const float* scales, const float* rotations, int raw,
                                    const float* viewmatrix, const float* campos, const float* dL_dnormals,
                                    float* dL_drotations, void* stream);

/* Bytes of device scratch r3dgs_depth_normal needs for the loss; 0 for an empty image.  A pure function of its arguments. */
size_t r3dgs_depth_normal_workspace_bytes(int H, int W);

/* depth [H*W]; alpha [H*W] or NULL -> surf_normal [3,H,W].  With normal_map [3,H,W] not NULL also the loss: pixel_weight
 * [H*W] or NULL, loss [1] on the device, workspace (8-byte aligned, not cleared).  One launch, two with the loss. */
int r3dgs_depth_normal(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                       const float* normal_map, const float* pixel_weight, int scale_by_alpha, float* surf_normal, float* loss,
                       char* workspace, void* stream);

/* The same inputs; dL_dloss [1] on the device (or NULL: zero; needs normal_map) and dL_dsurf [3,H,W] (or NULL: zero): the two
 * upstream gradients add.  Outputs (any may be NULL; each one given is overwritten, every element written): dL_ddepth [H*W],
 * dL_dalpha [H*W] (through the division only; needs alpha), dL_dnormal_map [3,H,W] (needs normal_map).  Gather form: every
 * pixel collects the shares of its four neighbours from a staged tile with a two-pixel halo and writes its own element only.
 * One launch. */
int r3dgs_depth_normal_backward(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                                const float* normal_map, const float* pixel_weight, int scale_by_alpha, const float* dL_dloss,
                                const float* dL_dsurf, float* dL_ddepth, float* dL_dalpha, float* dL_dnormal_map, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_NORMALS_H */
