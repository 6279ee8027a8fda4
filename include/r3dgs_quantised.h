/* r3dgs_quantised.h -- C ABI of the codebook-indexed (quantised) model: the inference forward that reads the compressed
 * representation in place, its decoder, and its size (reduced-3dgs_amd/csrc/quant_math.h, preprocess.hip, capi.hip,
 * pass_driver.hip).
 * The Python surface is r3dgs_quantised.QuantisedModel.
 * Same conventions as r3dgs_rasterizer.h: device pointers; `void* stream` is a hipStream_t; return >= 0 on success, < 0
 * with the message in r3dgs_last_error().  The forwards are inference only; what training needs beside them is the adjoint of
 * the lookup, r3dgs_quantised_codebook_grad below, which turns the gradients of the decoded tensors into the codebooks'.
 *
 * The model (what the reference's save_ply(quantised=True) stores, scene/gaussian_model.py:239-311), Gaussians sorted by
 * SH degree as in the file's vertex_0..vertex_3 groups; all arrays plain and contiguous:
 *   xyz         half [P,3] (IEEE binary16 bit patterns, xyz_is_half != 0) or float [P,3]
 *   geom_ids    uint8 [P,8]: opacity, scale x/y/z, rotation re, rotation im x/y/z.  8-byte aligned.
 *   sh_ids      uint8, ragged: Gaussian i of degree d owns 3 (d+1)^2 bytes in the order [coefficient][channel], the DC
 *               rgb first, at byte 3 * (the offset of the fp32 ragged buffer, in coefficients).  No padding is required:
 *               the kernels never read in front of the first byte or behind the last.
 *   codebooks   float [20][256], rows in the file's order: features_dc, features_rest_0..14, opacity, scaling,
 *               rotation_re, rotation_im (half centres widened once at load).  16-byte aligned.  Coefficient k >= 1 of
 *               all three channels reads features_rest_{k-1}, coefficient 0 features_dc.
 *   coeffsNum, perBandPrimitiveCount, cumSumPrimitiveCount: device int[4] each, as for r3dgs_inference_forward.
 * The codebooks hold the model's RAW parameters: opacity logits, log-scales, and a quaternion whose real and imaginary
 * parts were quantised apart; the kernels apply exp and the normalisation of r3dgs_forward_params after the lookup.
 * A lookup copies a float and every half is a float exactly, so the result equals, bit for bit, the forward of
 * r3dgs_inference_forward fed the tensors r3dgs_quantised_decode writes (scales / rotations through
 * r3dgs_activate_params). */
#ifndef R3DGS_QUANTISED_H
#define R3DGS_QUANTISED_H

#include <stddef.h>

#include "r3dgs_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r3dgs_inference_forward with the five model pointers replaced by the arrays above (and no precomputed colours or
 * covariances).  D is not read (the degree follows from the index) and may be NULL.  bandsNum must be 4.  The geometry
 * blob is the lean one (r3dgs_geometry_bytes_lean).  Returns num_rendered. */
int r3dgs_quantised_forward(r3dgs_alloc_fn geometryBuffer, void* geometry_user, r3dgs_alloc_fn binningBuffer, void* binning_user,
                            r3dgs_alloc_fn imageBuffer, void* image_user, int P, const int* D, int bandsNum,
                            const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                            const float* background, int width, int height, const void* xyz, int xyz_is_half,
                            const unsigned char* geom_ids, const unsigned char* sh_ids, const float* codebooks,
                            float scale_modifier, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                            float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* out_touched_pixels,
                            float* out_transmittance, int* radii, int calculate_mean_transmittance, int debug, void* stream);

/* r3dgs_inference_forward_reserved likewise: caller-provided blobs, a pair reservation, no host wait; returns the pass
 * ticket.  A replayed pass reads the model through its pointers when it runs: new contents give a new image. */
long long r3dgs_quantised_forward_reserved(char* geom_buffer, char* binning_buffer, char* image_buffer, int reserve, int P,
                                           const int* D, int bandsNum, const int* coeffsNum,
                                           const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                                           const float* background, int width, int height, const void* xyz, int xyz_is_half,
                                           const unsigned char* geom_ids, const unsigned char* sh_ids, const float* codebooks,
                                           float scale_modifier, const float* viewmatrix, const float* projmatrix,
                                           const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                                           float* out_color, int* out_touched_pixels, float* out_transmittance, int* radii,
                                           int calculate_mean_transmittance, int debug, void* stream);

/* The dense fp32 tensors the reference's load_ply returns for the model, written on the device by the functions the
 * forward's kernels use: xyz_out [P,3], features_dc [P,1,3], features_rest [P,15,3], opacity [P,1], scaling [P,3],
 * rotation [P,4], degrees [P,1].  Coefficients above a Gaussian's degree decode to centre 0 of their codebook, as the
 * reference's loader pads their index with 0.  Any output may be NULL. */
int r3dgs_quantised_decode(int P, const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                           const void* xyz, int xyz_is_half, const unsigned char* geom_ids, const unsigned char* sh_ids,
                           const float* codebooks, float* xyz_out, float* features_dc, float* features_rest, float* opacity,
                           float* scaling, float* rotation, int* degrees, void* stream);

/* The adjoint of r3dgs_quantised_decode in the codebooks: dL_dcodebooks float [20][256], rows in the order of `codebooks`;
 * centre c of book b receives the sum of the gradient elements whose id byte names it.  The five gradients are shaped exactly
 * as the decoder writes its outputs -- dL_dfeatures_dc [P,1,3], dL_dfeatures_rest [P,15,3], dL_dopacity [P,1], dL_dscaling
 * [P,3], dL_drotation [P,4] -- with the Gaussians in the model's own order (sorted by degree); any of them may be NULL and
 * then counts as zeros.  A Gaussian of degree d contributes its 8 geometry slots (opacity -> book 16, the three scales -> 17,
 * rotation re -> 18, the three rotation im -> 19) and the 3 (d+1)^2 SH slots it owns in sh_ids (coefficient 0 of all channels
 * -> book 0, coefficient k >= 1 -> book k).  Rows of dL_dfeatures_rest ABOVE the Gaussian's degree are NOT READ: the decoder
 * pads them with centre 0 of their book, and the rasterizer's gradient there is zero whenever lambda_sh_sparsity is 0.
 * All 5120 entries are overwritten by every call; a centre without a member gets +0.0.  Every sum is accumulated in double
 * in an order fixed by (P, the ids) and rounded to float once, without atomics: the same inputs give the same bits.  The
 * call only enqueues work on `stream` (graph-capturable, no host wait); its grid depends on P alone.
 * workspace: r3dgs_quantised_codebook_grad_workspace_bytes(P) bytes of device memory, 8-byte aligned, contents irrelevant
 * (0 bytes, and then possibly NULL, for P == 0). */
size_t r3dgs_quantised_codebook_grad_workspace_bytes(int P);
int r3dgs_quantised_codebook_grad(int P, const int* coeffsNum, const int* perBandPrimitiveCount, const int* cumSumPrimitiveCount,
                                  const unsigned char* geom_ids, const unsigned char* sh_ids, const float* dL_dfeatures_dc,
                                  const float* dL_dfeatures_rest, const float* dL_dopacity, const float* dL_dscaling,
                                  const float* dL_drotation, float* dL_dcodebooks, void* workspace, void* stream);

/* Resident bytes of a model: P (8 + 6 or 12) + sum_d 3 (d+1)^2 P_d + 20 * 256 * 4 + the three band tables (48).
 * perBandPrimitiveCount_host: HOST int[4], adding up to P.  0 with a message on bad arguments. */
size_t r3dgs_quantised_bytes(int P, const int* perBandPrimitiveCount_host, int xyz_is_half);

#ifdef __cplusplus
}
#endif

#endif /* R3DGS_QUANTISED_H */
