/* r3dgs_importance.h -- C ABI of the per-Gaussian blend-contribution scores: how much each Gaussian contributes to the
 * rendered pixels of a view, replayed from the three state blobs a forward pass left (reduced-3dgs_amd/csrc/importance.hip,
 * csrc/importance_math.h).  Same conventions as r3dgs_aux.h: device pointers, contiguous; `void* stream` is a hipStream_t;
 * return 0 on success, < 0 with the message in r3dgs_last_error().  No host wait, no allocation, no float atomics: the call
 * can be captured in a graph (query the workspace size outside the capture) and the same inputs give the same bits.
 *
 * A BLENDED entry of a pixel is an entry of its tile's list that passes the forward's own per-entry rule: among the first
 * n_contrib[pixel] entries (the forward's own count), not skipped on power > 0 or alpha < 1/255, alpha = min(0.99,
 * opacity * G), T <- T - alpha T.  Its blend weight is w = alpha * T_before (fp32, T running forward from 1 as the forward
 * runs it).  With an optional pixel weight map m [H, W] (NULL: all ones), per Gaussian g of ONE view:
 *   sum[g]   = sum of m[p] * w over the pixels p with m[p] != 0 that blend g
 *   max[g]   = the largest w over those same pixels (unweighted); 0 if there is none
 *   count[g] = the number of those pixels
 * A pixel with m[p] == 0 (either sign of zero) is masked out of all three: m is a region of interest as well as a weight.
 * Negative weights are allowed in sum.  No background term.  A Gaussian with radii == 0 (no pairs) gets zeros.  A Gaussian
 * that lost pairs to an overflowed pair reservation contributes nothing for that view, as r3dgs_aux_maps_backward gives it
 * zero rows.
 *
 * The blobs must be those of ONE forward over (P, width, height), any entry point, full or lean geometry blob, with R the
 * pair capacity of its binning blob (as r3dgs_aux_maps takes them).  They are only read. */
#ifndef R3DGS_IMPORTANCE_H
#define R3DGS_IMPORTANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace of r3dgs_contribution_scores (0 for P == 0 or R == 0; contents irrelevant before and after).
 * Per pair: 4 quadrants x 16 B rows (sum fp32, max fp32, count u32, 0) = 64 B, and 16 B of sort keys and values (two
 * uint32 each, before and after the sort); plus the sort's temporary storage. */
size_t r3dgs_contribution_scores_workspace_bytes(int P, int R, int width, int height);

/* pixel_weight: float [H*W] or NULL (all ones).
 * Outputs, each [P], any of them NULL (not computed): score_sum double, score_max float, score_count long long, score_views
 * int (the views in which count > 0).
 *   accumulate == 0: every row of every output is OVERWRITTEN (views with 0 or 1).
 *   accumulate == 1: the view is folded into what the buffers hold: sum += view_sum (one double added to one double),
 *     max = max(max, view_max), count += view_count, views += (view_count > 0).
 *   P == 0 or R == 0: with accumulate == 0 the outputs are zero-filled, with accumulate == 1 they are left alone; the blobs
 *     are not read in either case.
 * T_check float [H*W], n_check unsigned [H*W], either NULL: the walk's own final T and last contributor per pixel, which
 * equal the forward's final_T and n_contrib bit for bit (for tests; they ignore pixel_weight).
 * The walk's per-(pair, quadrant) rows are added per Gaussian in a fixed order (list slot ascending, quadrant 0..3). */
int r3dgs_contribution_scores(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                              const float* pixel_weight, double* score_sum, float* score_max, long long* score_count,
                              int* score_views, int accumulate, float* T_check, unsigned* n_check, char* workspace,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_IMPORTANCE_H */
