/* r3dgs_densify.h -- C ABI of densification: clone / split / prune of the Gaussians, of both Adam moments of every parameter
 * and of the per-Gaussian bookkeeping, as one read and one write of the state (scene/gaussian_model.py:502-522, :553-691 of
 * the reference: four cat / mask-index passes over every tensor and a dozen host waits).  Same conventions as
 * r3dgs_trainstats.h: device pointers, 4-byte elements, contiguous; `void* stream` is a hipStream_t; return >= 0 on success,
 * < 0 with the message in r3dgs_last_error().  Nothing here waits on the host or allocates.
 *
 * A call has two halves, with the caller's single read-back between them:
 *   1. r3dgs_densify_plan (or r3dgs_prune_plan): one flag byte per source Gaussian, the per-workgroup counts, their scan,
 *      the source row of every destination row -- all into `workspace` -- and eight int32 into `totals`:
 *        totals[0..3] = rows of segments A, B, C, D        totals[4] = n_points_cloned     totals[5] = n_points_split
 *        totals[6]    = n_points_pruned                    totals[7] = A + B + C + D (the new Gaussian count)
 *      The caller copies `totals` to the host -- the only wait, needed to size the destination tensors.
 *   2. r3dgs_densify_move: one launch that writes every destination tensor of the table.
 *
 * Destination order, every segment stable in source-index order:
 *   A  sources that are neither split nor pruned        C  surviving first children of the split sources
 *   B  surviving clones                                 D  surviving second children
 * The decisions, per source Gaussian (csrc/densify_math.h; thresholds are fp32, rounded once by the caller):
 *   grads = accum / denom, NaN -> 0;  scale = exp(scaling);  hot = densify and grads >= max_grad
 *   clone = hot and max scale <= dense_scale;  split = hot and max scale > dense_scale
 *   pruned = sigmoid(opacity) < min_opacity  or, with `screen`:  radii > max_screen  or  max scale > world_scale
 *     radii is max_radii2D[i] for densify == 0 and 0 for densify == 1 (the reference has zeroed it by then); a clone has its
 *     source's mask; a child has max exp(log(scale / 1.6)) for max scale and radii 0.
 */
#ifndef R3DGS_DENSIFY_H
#define R3DGS_DENSIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3DGS_DENSIFY_MAX_TENSORS 32
#define R3DGS_DENSIFY_TOTALS 8

/* How r3dgs_densify_move fills the rows of one tensor. */
#define R3DGS_DENSIFY_COPY 0      /* every row is its source's row (a parameter, _degrees, an accumulator of a bare prune) */
#define R3DGS_DENSIFY_ZERO_NEW 1  /* segment A: the source's row; B, C, D: zeros (exp_avg, exp_avg_sq, a stored .grad) */
#define R3DGS_DENSIFY_XYZ 2       /* A, B: the source's row; C, D: R(rotation) (noise * exp(scaling)) + xyz; 3 words per row */
#define R3DGS_DENSIFY_SCALING 3   /* A, B: the source's row; C, D: log(exp(scaling) / 1.6); 3 words per row */

typedef struct {
    const void* src; /* [P, row_words] 4-byte elements */
    void* dst;       /* [totals[7], row_words] */
    int row_words;   /* 4-byte words per row; 0: the tensor has no columns and is skipped */
    int kind;        /* R3DGS_DENSIFY_* */
} r3dgs_densify_tensor;

/* Bytes of device scratch a plan for P source Gaussians needs, shared by plan and move; 0 for P <= 0.  A pure function of P. */
size_t r3dgs_densify_workspace_bytes(int P);

/* The plan of densify_and_prune (densify = 1) or of prune() on its own (densify = 0).  accum, denom: xyz_gradient_accum and
 * denom, fp32 [P] (read only for densify = 1); scaling: raw fp32 [P,3]; opacity: raw fp32 [P]; max_radii2D: fp32 [P] (read
 * only for densify = 0 with screen != 0).  max_grad must be > 0 for densify = 1: the reference takes the split decision on
 * the set the clones were appended to with a zero gradient, so max_grad <= 0 would split the clones.
 * workspace: r3dgs_densify_workspace_bytes(P) bytes, 16-byte aligned, not cleared; totals: int32 [8] on the device. */
int r3dgs_densify_plan(int P, int densify, const float* accum, const float* denom, const float* scaling, const float* opacity,
                       const float* max_radii2D, float max_grad, float dense_scale, float min_opacity, int screen,
                       float max_screen, float world_scale, char* workspace, int* totals, void* stream);

/* The plan of prune_points(mask): mask is uint8 [P] (a torch bool tensor), non-zero = remove.  Only segment A has rows;
 * totals[6] counts the removed ones. */
int r3dgs_prune_plan(int P, const uint8_t* mask, char* workspace, int* totals, void* stream);

/* Writes the n tensors of the table from the plan in `workspace`.  nA, nB, nC: totals[0..2] as the caller read them
 * (D has nC rows).  xyz, scaling, rotation: the source parameters [P,3], [P,3], [P,4] and noise: standard-normal fp32
 * [2, P, 3] indexed by (child, source Gaussian) -- read only for the rows of segments C and D, required when nC > 0.
 * A destination row gathers its source row; the destination index runs along the lanes, and 16-byte loads and stores are used
 * wherever the destination base, the source address of a row and the row width allow.  No atomics: the output is a function
 * of the inputs alone. */
int r3dgs_densify_move(int P, int nA, int nB, int nC, int n, const r3dgs_densify_tensor* tensors, const float* xyz,
                       const float* scaling, const float* rotation, const float* noise, const char* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_DENSIFY_H */
