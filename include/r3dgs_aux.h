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
 * The maps carry no gradient.
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

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_AUX_H */
