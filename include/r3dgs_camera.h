/* r3dgs_camera.h -- C ABI of the camera gradients: dL/dviewmatrix, dL/dprojmatrix and dL/dcampos of a rendered image, from
 * the per-Gaussian screen-space sums a backward pass has just written (reduced-3dgs_amd/csrc/camera_bwd.hip, csrc/camera_math.h).
 * Same conventions as r3dgs_rasterizer.h: device pointers, fp32 / int32, contiguous; `void* stream` is a hipStream_t; return 0
 * on success, < 0 with the message in r3dgs_last_error().
 *
 * The three camera arrays are treated as INDEPENDENT inputs: the outputs are partial derivatives, output entry k is
 * dL/d(input[k]) in the layout of the input -- the transposed, row-vector matrices exactly as r3dgs_forward takes them -- and
 * the caller chains them through whatever ties the three together (a pose parameterisation: r3dgs_camera.RefinedCamera).
 * With mt = [m, 1], per Gaussian with radii > 0 and with r3dgs_backward's conventions throughout:
 *   projmatrix  enters through h = mt F and the pixel mean only: dL_dmean2D (x, y; the third component takes no part), in
 *               the units r3dgs_backward writes it, goes back through 1 / (h.w + 1e-7) to dL/dh, and the Gaussian adds the
 *               outer product mt^T dL/dh.  Column 2 of F is never read: its gradient is zero.
 *   viewmatrix  enters through t = mt V inside the Jacobian J(t), and through the rotation Rw = V[:3,:3]^T in
 *               cov2D = (J Rw) Sigma (J Rw)^T: dL_dconic is chained to cov2D (the + 0.3 blur and 1 / (det^2 + 1e-7) as
 *               r3dgs_backward treats them), then to J and Rw.  A clamped t.x / t.z or t.y / t.z passes nothing along that
 *               path.  The chain runs in double or in fp32 as r3dgs_set_f64_chain says.  Column 3 of V is never read: its
 *               gradient is zero.  The depth order, the cull, the radius and the tile rect are integer decisions.
 *   campos      enters through the SH view direction d = m - campos only:
 *               dL/dcampos = - sum (I - dn dn^T) / |d| (d rgb / d dn)^T dL_dcolor, dn = d / |d|, a colour channel the forward
 *               clamped at 0 left out.  d rgb / d dn is taken from the forward's state when its header says it is there
 *               (dense SH, a forward that trained), else evaluated from the SH row with the row's own degree.  Zero for
 *               precomputed colours (shs == NULL).
 * What is NOT differentiated: tan_fovx / tan_fovy (the focal lengths of the Jacobian and of the clamp).
 *
 *   P, D [P] degrees, M: as r3dgs_backward.  means3D [P,3].
 *   raw_params == 0: shs [P,M,3] or NULL (precomputed colours), shs_rest ignored; scales [P,3] / rotations [P,4] ACTIVATED,
 *     or cov3D_precomp [P,6] (the two may then be NULL).
 *   raw_params == 1 (behind r3dgs_backward_params): shs = features_dc [P,1,3], shs_rest = features_rest [P,M-1,3] (NULL iff
 *     M == 1), scales / rotations the model's raw _scaling / _rotation, activated in the kernel by the functions the
 *     raw-parameter passes use; cov3D_precomp must be NULL.
 *   viewmatrix, projmatrix [16], campos [3], tan_fovx, tan_fovy, width, height, scale_modifier: the forward's.
 *   radii [P] as the forward returned them; geom_buffer: the forward's geometry blob (read only: the clamp bits, the tile
 *     counts, the header and, if present, the SH direction derivatives).
 *   dL_dmean2D [P,3], dL_dconic [P,4] (A, B, -, C), dL_dcolor [P,3]: as r3dgs_backward / r3dgs_backward_params just wrote them.
 *   dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3]: any may be NULL (not written).  OVERWRITTEN, every element, the
 *     structurally empty columns with zeros.
 *   workspace: r3dgs_camera_backward_workspace_bytes(P) bytes of device memory, contents irrelevant before and after.
 *
 * Two launches on `stream`: one pass over the Gaussians (one lane per Gaussian per trip, culled rows skipped before any of
 * their other loads, 27 double sums per lane, one row of partial sums per workgroup into the workspace) and a one-workgroup
 * finish that adds the rows in index order.  The grid depends on P alone and there are no atomics: the same inputs give the
 * same bits.  No host wait, no allocation: the call can be captured in a graph (query the workspace size outside the capture).
 * A degree in D above what M coefficients support is taken as the degree they do support.
 * P == 0: the outputs are zero-filled and nothing is read.  Nothing visible: zeros; of the per-Gaussian arrays only radii is
 * read (every workgroup also reads the 35 camera words and the sh_cache word of the blob's header before its loop). */
#ifndef R3DGS_CAMERA_H
#define R3DGS_CAMERA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t r3dgs_camera_backward_workspace_bytes(int P);
int r3dgs_camera_backward(int P, const int* D, int M, int width, int height, const float* means3D, const float* shs,
                          const float* shs_rest, const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, int raw_params, const float* viewmatrix, const float* projmatrix,
                          const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                          const float* dL_dmean2D, const float* dL_dconic, const float* dL_dcolor, float* dL_dviewmatrix,
                          float* dL_dprojmatrix, float* dL_dcampos, char* workspace, void* stream);

/* The camera pass of the replay maps: dL/dviewmatrix and dL/dprojmatrix of a loss on the depth / alpha / median-depth maps
 * (r3dgs_aux.h), the distortion map (r3dgs_distortion.h) or a feature map (r3dgs_features.h), from the per-Gaussian
 * screen-space sums the map's _screen backward has just written (r3dgs_aux_maps_backward_screen,
 * r3dgs_distortion_backward_screen, r3dgs_feature_maps_backward_screen).  Conventions, layouts and the partial-derivative
 * reading of the outputs as r3dgs_camera_backward; per Gaussian with radii > 0 and mt = [m, 1]:
 *   projmatrix  from dL_dmean2D, as above;
 *   viewmatrix  from dL_dconic through J(t) and Rw, as above (the clamp masks are taken again in fp32 as the forward took
 *               them: the geometry blob is not read), and -- the one path a colour image does not have -- from dL_dz: the maps
 *               read the view depth z = (mt V)_2 itself, so dL_dviewmatrix[4 k + 2] += dL_dz * mt[k];
 *   there is no campos output: no SH direction is involved.  tan_fovx / tan_fovy are not differentiated.
 *   means3D [P,3]; scales [P,3] / rotations [P,4] ACTIVATED, or cov3D_precomp [P,6] (the two may then be NULL);
 *   viewmatrix, projmatrix [16], tan_fovx, tan_fovy, width, height, scale_modifier: the forward's; radii [P] as it returned them.
 *   dL_dmean2D [P,3] (x, y; the third component takes no part), dL_dconic [P,4] (A, B, -, C), dL_dz [P]: any of them NULL = zero.
 *   dL_dviewmatrix [16], dL_dprojmatrix [16]: either may be NULL (not written).  OVERWRITTEN, every element, column 3 of the
 *     first and column 2 of the second with zeros.
 *   workspace: r3dgs_camera_backward_maps_workspace_bytes(P) bytes of device memory, contents irrelevant before and after.
 * Two launches on `stream`: a kernel of its own over the Gaussians (one lane per Gaussian per trip, radii loaded first and
 * everything else only where radii > 0, 24 double sums per lane, the wave / workgroup reduction of r3dgs_camera_backward in
 * its fixed order, one row per workgroup into the workspace) and r3dgs_camera_backward's one-workgroup finish.  No SH loads,
 * no atomics, no host wait, no allocation: the same inputs give the same bits, and the call can be captured in a graph (query
 * the workspace size outside the capture).  The chain runs in double or in fp32 as r3dgs_set_f64_chain says.
 * P == 0, or all three gradient inputs NULL: the outputs are zero-filled and nothing is read.  Each map runs its own pass and
 * the caller adds the shares (autograd does): the pass is linear in its three gradient inputs. */
size_t r3dgs_camera_backward_maps_workspace_bytes(int P);
int r3dgs_camera_backward_maps(int P, int width, int height, const float* means3D, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                               const float* projmatrix, float tan_fovx, float tan_fovy, const int* radii,
                               const float* dL_dmean2D, const float* dL_dconic, const float* dL_dz, float* dL_dviewmatrix,
                               float* dL_dprojmatrix, char* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_CAMERA_H */
