/* r3dgs_features.h -- C ABI of the per-Gaussian feature maps: an arbitrary feature vector F[P, C] blended into a [C, H, W]
 * map, replayed from the three state blobs a forward pass left, with gradients (reduced-3dgs_amd/csrc/feature_maps.hip,
 * csrc/feature_math.h).  Same conventions as r3dgs_aux.h: device pointers, fp32, contiguous; `void* stream` is a hipStream_t;
 * return 0 on success, < 0 with the message in r3dgs_last_error().  No host wait, no allocation, no float atomics: the calls
 * can be captured in a graph (query the workspace size outside the capture) and their results are identical run to run.
 *
 * Per pixel, over the first n_contrib[pixel] entries of its tile's list (the forward's own count), with the forward's
 * per-entry rule (skip on power > 0 or alpha < 1/255, alpha = min(0.99, opacity * G), T <- T - alpha T):
 *   out[c, pixel]   = sum_k F[id_k, c] * alpha_k * T_before_k      fp32, in list order, accumulated as a colour channel is
 *   dL/dF[id_k, c] += alpha_k T_k g[c, pixel]
 *   dL/dalpha_k     = sum_c g[c, pixel] (F[id_k, c] T_k - S_kc / (1 - alpha_k)),   S_kc = sum_{j > k} F[id_j, c] alpha_j T_j
 * No background term and no normalisation (divide by the alpha map for a mean); a pixel nothing contributed to gets 0.  The
 * backward walks back to front with T recovered from final_T by division, as the colour backward recovers it; the clamp at
 * 0.99 does not stop the gradient; from dL/dalpha_k onwards the chain is the colour backward's (through G to the conic and the
 * pixel mean, through o to the raw opacity; the covariance chain in double or fp32 as r3dgs_set_f64_chain says).
 *
 * 1 <= C <= R3DGS_FEATURE_MAX_CHANNELS; any other C is refused with a message.  The blobs must be those of ONE forward over
 * (P, width, height), any entry point, full or lean geometry blob, with R the pair capacity of its binning blob (as
 * r3dgs_aux_maps takes them).  They are only read: a colour backward over them afterwards gives what it gives without these
 * calls. */
#ifndef R3DGS_FEATURES_H
#define R3DGS_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#define R3DGS_FEATURE_MAX_CHANNELS 512

#ifdef __cplusplus
extern "C" {
#endif

/* features [P, C] -> out [C, H, W].  P == 0 or R == 0: out is zero-filled and the blobs are not read. */
int r3dgs_feature_maps(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                       const float* features, int C, float* out, void* stream);

/* Gradients through the map: dL_dout [C, H, W] -> dL_dfeatures [P, C] and the geometry gradients r3dgs_aux_maps_backward
 * writes, in its units and with its inputs (means3D [P,3]; scales [P,3] and rotations [P,4] ACTIVATED, or cov3D_precomp [P,6];
 * radii [P] as the forward returned them; viewmatrix, projmatrix [16]).
 *   Any output may be NULL (not computed).  With every geometry output NULL (frozen geometry) the geometric sums, their
 *   workspace rows and the per-Gaussian chain are skipped altogether, and the camera and geometry inputs may be NULL.
 *   The outputs are OVERWRITTEN; every row is written; a row with radii == 0 gets zeros.
 *   P == 0, R == 0 or dL_dout == NULL: the outputs are zero-filled and the blobs are not read.
 *   A Gaussian that lost pairs to an overflowed reservation gets zero rows, as r3dgs_aux_maps_backward gives it.
 * workspace: r3dgs_feature_maps_backward_workspace_bytes(P, R, C, width, height) bytes of device memory (an upper bound over
 *   the NULL combinations; 0 for P == 0 or R == 0), contents irrelevant before and after.  With G = ceil(C / 16) channel
 *   groups, per pair: 4 quadrants x G x 64 B of feature sums, 4 x G x 32 B of geometric sums, 16 B of sort keys and values
 *   (384 G + 16 bytes), plus the sort's temp storage. */
size_t r3dgs_feature_maps_backward_workspace_bytes(int P, int R, int C, int width, int height);
int r3dgs_feature_maps_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                                const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                                const float* cov3D_precomp, const int* radii, const float* features, int C, const float* dL_dout,
                                float* dL_dfeatures, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity,
                                float* dL_dscales, float* dL_drotations, float* dL_dcov3D, char* workspace, void* stream);

/* r3dgs_feature_maps_backward that also hands out the screen-space sums its per-Gaussian chain starts from, for the camera
 * pass of the maps (r3dgs_camera.h r3dgs_camera_backward_maps).  Everything as above -- the same workspace, the seven outputs
 * the same bits -- plus two optional outputs, as r3dgs_aux_maps_backward_screen has them:
 *   dL_dconic [P,4]  A, B, unused (written 0), C, in the layout and units r3dgs_camera_backward reads
 *   dL_dz [P]        zeros: a feature map does not read the view depth (written so that the three _screen calls are alike)
 * Zero rows for culled Gaussians and for those that lost pairs.  Both NULL: the call IS r3dgs_feature_maps_backward.  One of
 * them asked for and dL_dmeans3D .. dL_dcov3D all NULL (a frozen model): the geometric sums are still walked (features must
 * not be NULL), the chain behind them is skipped and viewmatrix .. cov3D_precomp may be NULL. */
int r3dgs_feature_maps_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                       char* image_buffer, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                                       float tan_fovy, const float* means3D, const float* scales, float scale_modifier,
                                       const float* rotations, const float* cov3D_precomp, const int* radii,
                                       const float* features, int C, const float* dL_dout, float* dL_dfeatures,
                                       float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales,
                                       float* dL_drotations, float* dL_dcov3D, float* dL_dconic, float* dL_dz, char* workspace,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_FEATURES_H */
