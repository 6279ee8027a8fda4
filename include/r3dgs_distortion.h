/* r3dgs_distortion.h -- C ABI of the depth-distortion map, the second geometry regulariser of 2DGS / GOF / PGSR / RaDe-GS, and
 * of the gradients through it, replayed from the three state blobs a forward pass left (reduced-3dgs_amd/csrc/distortion.hip,
 * csrc/distortion_math.h).  Same conventions as r3dgs_rasterizer.h and r3dgs_aux.h: device pointers, fp32 / uint32,
 * contiguous; `void* stream` is a hipStream_t; return 0 on success, < 0 with the message in r3dgs_last_error().
 *
 * Definition: the SQUARED form, as 2DGS's rasterizer computes it.  Per pixel, over the first n_contrib[pixel] entries of its
 * tile's list (the forward's own count, so the stop is the forward's stop), with the forward's per-entry rule (skip on power > 0
 * or alpha < 1/255, alpha = min(0.99, opacity * G), T <- T - alpha T), exactly as r3dgs_aux_maps walks them; w_k = alpha_k *
 * T_before_k the blend weight and m_k the mapped depth of entry k:
 *   distortion [H*W] = sum_k w_k (m_k^2 A_<k + D2_<k - 2 m_k D1_<k) = sum_{j<k} w_j w_k (m_k - m_j)^2
 *                      A_<k = sum_{j<k} w_j,  D1_<k = sum_{j<k} w_j m_j,  D2_<k = sum_{j<k} w_j m_j^2
 *   There is no background term; a pixel nothing contributed to gets 0.
 * The depth mapping is selected by (near, far):
 *   near = far = 0 : linear, m = z, the view-space depth
 *   0 < near < far : 2DGS's, m = far / (far - near) * (1 - near / z), dm/dz = far near / ((far - near) z^2)
 *   anything else returns < 0 with a message.
 * (The linear-ORDER form of Mip-NeRF 360 and gsplat, sum w_j w_k |m_k - m_j|, is not computed.)
 * Depths are carried relative to the mapped depth of the tile's first list entry (every expression is invariant under the
 * shift), the running sums in double, so that depths around 100 with a spread around 1 keep the answer.  The view depths are
 * taken as the forward left them and are not checked: every Gaussian a forward bins has passed its near cull (view depth
 * z > 0.2), so z and the reference depth are positive and 2DGS's mapping and its shifted form (z - z_ref) / (z z_ref) are finite.
 *   saved_moments [2, H*W] or NULL: the pixel's totals S1 = sum w m and S2 = sum w m^2 over the SHIFTED mapped depths; what
 *   r3dgs_distortion_map_backward reads (the third total, A = sum w, is 1 - final_T of the forward).
 * r3dgs_distortion_map is one kernel launch on `stream` (memsets when there is nothing to walk): no host wait, no allocation,
 * no atomics -- it can be captured in a graph and its results are identical run to run.  Either output may be NULL (not
 * computed).  P == 0 or R == 0: the outputs are zero-filled and the blobs are not read.  Otherwise the three blobs must be those
 * of ONE forward over (P, width, height) -- r3dgs_forward (exact or reserved), r3dgs_forward_params, r3dgs_inference_forward,
 * r3dgs_quantised_forward, full or lean geometry blob -- with R the pair capacity its binning blob was carved with.  The blobs
 * are only read: a backward over them afterwards gives what it gives without this call. */
#ifndef R3DGS_DISTORTION_H
#define R3DGS_DISTORTION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int r3dgs_distortion_map(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                         float near, float far, float* distortion, float* saved_moments, void* stream);

/* Gradients THROUGH the map: the upstream gradient dL_ddistortion [H*W] -> gradients of the Gaussians, over the same three
 * blobs (read only) and the saved_moments of r3dgs_distortion_map over them with the same (near, far).
 *
 * With the pixel's totals A = 1 - final_T, S1, S2:
 *   distortion         = A S2 - S1^2
 *   d dist / d w_k     = A m_k^2 - 2 m_k S1 + S2 = sum_j w_j (m_k - m_j)^2     (c_k)
 *   d dist / d m_k     = 2 w_k (A m_k - S1)
 * w_k depends on the alphas in front of it as a colour channel's weight does: per pixel the pass walks the entries the forward
 * blended back to front, T recovered from final_T by division, and dL/dalpha_k is the colour backward's step on a splat of
 * colour c_k under the pixel gradient dL_ddistortion over a black background; the view depth z_k receives dL_ddistortion *
 * 2 w_k (A m_k - S1) * dm/dz.  From there on everything is r3dgs_aux_maps_backward's, with its conventions: seven sums per
 * (pair, 8x8 quadrant) in a slab, a stable sort by Gaussian id, fixed-order sums in double, the per-Gaussian chain in double or
 * fp32 as r3dgs_set_f64_chain says, the clamp at 0.99 does not stop the gradient, zeros for a Gaussian that lost pairs to an
 * overflowed reservation; z reaches means3D through the third row of viewmatrix.
 *   Inputs and outputs as r3dgs_aux_maps_backward: means3D [P,3]; scales [P,3] and rotations [P,4] ACTIVATED, or cov3D_precomp
 *   [P,6]; radii [P]; viewmatrix, projmatrix [16]; dL_dmeans2D [P,3], dL_dmeans3D [P,3], dL_dopacity [P,1] (of the RAW
 *   opacity), dL_dscales [P,3], dL_drotations [P,4], dL_dcov3D [P,6].  Any output may be NULL; the outputs are OVERWRITTEN.
 * workspace: r3dgs_distortion_map_backward_workspace_bytes(P, R, width, height) bytes of device memory (0 for P == 0 or
 *   R == 0; the layout of r3dgs_aux_maps_backward's), contents irrelevant before and after.
 * No float atomics, no host wait, no allocation: the call can be captured in a graph (query the workspace size outside the
 * capture first) and is bit-identical run to run.
 * P == 0: nothing is written.  R == 0 or dL_ddistortion NULL: the outputs are zero-filled and the blobs are not read.
 * Otherwise saved_moments must not be NULL. */
size_t r3dgs_distortion_map_backward_workspace_bytes(int P, int R, int width, int height);
int r3dgs_distortion_map_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                  char* image_buffer, float near, float far, const float* viewmatrix, const float* projmatrix,
                                  float tan_fovx, float tan_fovy, const float* means3D, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp, const int* radii,
                                  const float* dL_ddistortion, const float* saved_moments, float* dL_dmeans2D,
                                  float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                                  float* dL_dcov3D, char* workspace, void* stream);

/* r3dgs_distortion_map_backward that also hands out the screen-space sums its per-Gaussian chain starts from, for the camera
 * pass of the maps (r3dgs_camera.h r3dgs_camera_backward_maps).  Everything as above -- the same workspace, the six outputs
 * the same bits -- plus two optional outputs, as r3dgs_aux_maps_backward_screen has them:
 *   dL_dconic [P,4]  A, B, unused (written 0), C, in the layout and units r3dgs_camera_backward reads
 *   dL_dz [P]        the gradient of the view depth z alone: for 0 < near < far AFTER dm / dz of the mapping
 * Zero rows for culled Gaussians and for those that lost pairs.  Both NULL: the call IS r3dgs_distortion_map_backward.  One of
 * them asked for and dL_dmeans3D .. dL_dcov3D all NULL (a frozen model): the call still walks, the chain behind the
 * screen-space sums is skipped and viewmatrix .. cov3D_precomp may be NULL (radii and saved_moments may not). */
int r3dgs_distortion_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                     char* image_buffer, float near, float far, const float* viewmatrix, const float* projmatrix,
                                     float tan_fovx, float tan_fovy, const float* means3D, const float* scales,
                                     float scale_modifier, const float* rotations, const float* cov3D_precomp, const int* radii,
                                     const float* dL_ddistortion, const float* saved_moments, float* dL_dmeans2D,
                                     float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                                     float* dL_dcov3D, float* dL_dconic, float* dL_dz, char* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_DISTORTION_H */
