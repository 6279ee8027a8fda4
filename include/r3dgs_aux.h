/* r3dgs_aux.h -- C ABI of the auxiliary per-pixel maps: expected depth, accumulated opacity (alpha) and median depth,
 * replayed from the three state blobs a forward pass left (reduced-3dgs_amd/csrc/aux_maps.hip, csrc/aux_math.h).
 * Same conventions as r3dgs_rasterizer.h: device pointers, fp32 / uint32, contiguous; `void* stream` is a hipStream_t;
 * return 0 on success, < 0 with the message in r3dgs_last_error().  The call is one kernel launch on `stream` (memsets
 * when there is nothing to walk): no host wait, no allocation, no atomics -- it can be captured in a graph and its results
 * are identical run to run.
 *
 * Per pixel, over the first n_contrib[pixel] entries of its tile's list (the forward's own count, so the stop is the
 * forward's stop), with the forward's per-entry rule (skip on power > 0 or alpha < 1/255, alpha = min(0.99, opacity * G),
 * T <- T - alpha T) and z_k the view-space depth of entry k:
 *   depth        [H*W]  sum over the blended entries of z_k * alpha_k * T_before_k: fp32, in list order, accumulated as a
 *                       colour channel is.  NOT normalised and without a background term: divide by alpha for a mean depth.
 *   alpha        [H*W]  1 - final_T, from the final transmittance the forward stored
 *   median_depth [H*W]  z_k of the first blended entry after which T < 0.5; 0 if no entry brings T below 0.5
 *   a pixel nothing contributed to gets 0 in all three.
 * The maps themselves are plain arrays; r3dgs_aux_maps_backward below carries gradients through them.
 *   T_check [H*W] fp32 / n_check [H*W] uint32: the pass's OWN recomputed final transmittance and 1-based position of the
 *     last contributor; they equal the forward's final_T / n_contrib bit for bit (tests hold them to it).
 * Any output pointer may be NULL (not computed).  P == 0 or R == 0: the outputs are zero-filled and the blobs are not read.
 * Otherwise the three blobs must be those of ONE forward over (P, width, height) -- r3dgs_forward (exact or reserved),
 * r3dgs_forward_params, r3dgs_inference_forward, r3dgs_quantised_forward, full or lean geometry blob -- with R the pair
 * capacity its binning blob was carved with, as r3dgs_backward takes it.  The blobs are only read: a backward over them
 * afterwards gives what it gives without this call. */
#ifndef R3DGS_AUX_H
#define R3DGS_AUX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int r3dgs_aux_maps(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                   float* depth, float* alpha, float* median_depth, float* T_check, unsigned* n_check, void* stream);

/* Gradients THROUGH the maps: upstream gradients dL_ddepth, dL_dalpha, dL_dmedian (each [H*W], any of them NULL = zero) of
 * the three maps above -> gradients of the Gaussians, over the same three blobs (read only, as above).
 *
 * Per pixel the pass walks the entries the forward blended, back to front -- the forward's skip rule, nothing behind
 * n_contrib[pixel], T recovered from the forward's final_T by division as the colour backward recovers it -- with
 *   d depth / d z_k     = alpha_k T_k
 *   d depth / d alpha_k = z_k T_k - (sum_{j > k} z_j alpha_j T_j) / (1 - alpha_k)
 *   d alpha / d alpha_k = T_final / (1 - alpha_k)
 *   median_depth passes dL_dmedian to the z of the Gaussian it selected and to nothing else (the selection is piecewise
 *   constant); there is no background term, as in the maps.
 * This is the colour backward's step on a splat of colour (z, 1, 0) with the pixel gradient (dL_ddepth, dL_dalpha, 0) over a
 * black background.  From dL/dalpha_k onwards the chain is the colour backward's, with its conventions: alpha = min(0.99, o G),
 * the clamp does not stop the gradient, through G to the conic and the pixel mean and through o to the opacity; z is the
 * view-space depth and its gradient reaches means3D through the third row of viewmatrix.  The covariance chain runs in double
 * or in fp32 as r3dgs_set_f64_chain says, as r3dgs_backward's does.
 *   means3D [P,3]; scales [P,3] and rotations [P,4] ACTIVATED (what r3dgs_forward takes), or cov3D_precomp [P,6] (the others
 *   may then be NULL); radii [P] as the forward returned them (a row with radii == 0 gets zeros); viewmatrix, projmatrix [16].
 *   dL_dmeans2D [P,3]  gradient of the screen-space mean in the units r3dgs_backward writes (what densification reads; z = 0)
 *   dL_dmeans3D [P,3], dL_dopacity [P,1] (of the RAW opacity), dL_dscales [P,3], dL_drotations [P,4], dL_dcov3D [P,6]
 *   Any output may be NULL (not written).  The outputs are OVERWRITTEN, not added to; every row is written.
 * workspace: r3dgs_aux_maps_backward_workspace_bytes(P, R, width, height) bytes of device memory (0 for P == 0 or R == 0),
 *   contents irrelevant before and after: per (list slot, 8x8 quadrant) one 32-byte row of seven sums (2 pixel mean, 3 conic,
 *   1 opacity, 1 z) = 128 B per pair, four 4-byte arrays per pair for a stable radix sort of (Gaussian id, list slot), and the
 *   sort's temp storage.  Each Gaussian adds its rows in sorted order in double: no float atomics, bit-identical run to run.
 * A pass whose forward overflowed its pair reservation (num_rendered > R: the farthest pairs were dropped) gives a Gaussian that
 * lost pairs zero gradients instead of a partial sum, as r3dgs_backward does.
 * No host wait, no allocation: the call can be captured in a graph (query the workspace size outside the capture first).
 * P == 0 or R == 0, or all three upstream pointers NULL: the outputs are zero-filled and the blobs are not read. */
size_t r3dgs_aux_maps_backward_workspace_bytes(int P, int R, int width, int height);
int r3dgs_aux_maps_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                            const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                            const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, const int* radii, const float* dL_ddepth, const float* dL_dalpha,
                            const float* dL_dmedian, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity,
                            float* dL_dscales, float* dL_drotations, float* dL_dcov3D, char* workspace, void* stream);

/* r3dgs_aux_maps_backward that also hands out the screen-space sums its per-Gaussian chain starts from, for the camera pass
 * of the maps (r3dgs_camera.h r3dgs_camera_backward_maps, which reads them next to dL_dmeans2D).  Everything as above -- the
 * same workspace, the six outputs the same bits -- plus two optional outputs:
 *   dL_dconic [P,4]  A, B, unused (written 0), C: the gradient of the conic in the layout and units r3dgs_camera_backward
 *                    reads, i.e. what the chain feeds to its covariance backward
 *   dL_dz [P]        the gradient of the view depth z alone (what reaches means3D through the third row of viewmatrix)
 * Rows of culled Gaussians, and of Gaussians that lost pairs to an overflowed reservation, are zero.  With both NULL the call
 * IS r3dgs_aux_maps_backward.  With one of them asked for and dL_dmeans3D .. dL_dcov3D all NULL (a frozen model: a tracker
 * that fits the camera alone) the call still walks, the chain behind the screen-space sums is skipped and of the model only
 * radii is read: viewmatrix .. cov3D_precomp may be NULL. */
int r3dgs_aux_maps_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                   char* image_buffer, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                                   float tan_fovy, const float* means3D, const float* scales, float scale_modifier,
                                   const float* rotations, const float* cov3D_precomp, const int* radii, const float* dL_ddepth,
                                   const float* dL_dalpha, const float* dL_dmedian, float* dL_dmeans2D, float* dL_dmeans3D,
                                   float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                   float* dL_dconic, float* dL_dz, char* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_AUX_H */
