/* r3dgs_mcmc.h -- C ABI of the fixed-budget densification strategy of 3DGS-MCMC (Kheradmand et al., 2024): dead Gaussians are
 * relocated onto live ones, the model grows by a fixed factor up to a hard cap, and an opacity-gated, covariance-shaped noise
 * term moves the positions every iteration.  This is NOT the reference's densify_and_prune (r3dgs_densify.h); it stands beside
 * it.  Same conventions as r3dgs_densify.h: device pointers, 4-byte elements, contiguous; `void* stream` is a hipStream_t;
 * return >= 0 on success, < 0 with the message in r3dgs_last_error().  Nothing here allocates, waits on the host or uses a
 * float atomic: every output is a function of the inputs alone.  The activations are the library's own (sigmoid, exp,
 * normalised quaternion: csrc/stats_math.h, csrc/param_math.h); the per-Gaussian arithmetic is csrc/mcmc_math.h.
 *
 * Noise (every iteration), in place on xyz:
 *   o = sigmoid(opacity_raw)   gate = 1 / (1 + exp(-100 ((1 - o) - 0.995)))   S = R(q) diag(exp(scaling_raw))^2 R(q)^T
 *   xyz += scale * gate * (S noise_row)          a zero noise row leaves the bits of its xyz row as they were
 *
 * Plan (relocation and growth share it):
 *   w_i = sigmoid(opacity_raw_i); in R3DGS_MCMC_RELOCATE a Gaussian with w_i <= min_opacity is dead and has weight 0, in
 *   R3DGS_MCMC_GROW nobody is dead.  cdf = inclusive prefix sum of the weights in double, in a fixed order.  Draw k is the first
 *   index j with cdf[j] > uniforms[k] * cdf[P-1]; the search runs over the rows of positive weight only, so a row of weight 0
 *   is never drawn, whatever u in [0,1) is.  RELOCATE draws once per dead row (counted on the device; uniforms has P entries, the
 *   first n_dead are read) and slots[k] is the k-th dead row in index order; GROW draws n_draws times.
 *   ratio[i] = 1 + (times i was drawn), clamped to R3DGS_MCMC_MAX_RATIO.
 *   totals[0] dead rows          totals[1] draws made        totals[2] distinct sources      totals[3] sources whose ratio was clamped
 *   totals[4] 0: the plan acts, 1: nothing has positive weight, 2: nothing to draw (RELOCATE: nothing dead; GROW: n_draws == 0)
 *   totals[5] rows of positive weight                         totals[6..7] 0
 *   A plan with totals[4] != 0 is a no-op: ratio is all 1, totals[1] is 0.  (GROW with totals[4] == 1 -- every sigmoid
 *   underflowed to 0 -- still fills sampled[k] = k mod P, so that the grown rows are plain copies.)
 *
 * Move.  A drawn source with activated opacity o, scales s and ratio N >= 2 is rewritten as
 *   o' = 1 - (1 - o)^(1/N)      D = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)      s' = (o / D) s
 *   opacity_raw = logit(clamp(o', min_opacity, 1 - 2^-23))       scaling_raw = log(s')
 *   with o' and D in double from a table of exact binomials, rounded to fp32 once.
 *   RELOCATE, in place (src == dst in every table entry): every drawn source takes its new opacity and scaling, and row
 *   slots[k] becomes a copy of the updated row sampled[k].  GROW: dst has P + n_new rows; rows [0,P) are the old rows with the
 *   drawn sources updated and row P + k is a copy of the updated row sampled[k].
 */
#ifndef R3DGS_MCMC_H
#define R3DGS_MCMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3DGS_MCMC_MAX_TENSORS 32
#define R3DGS_MCMC_TOTALS 8
#define R3DGS_MCMC_MAX_RATIO 51

#define R3DGS_MCMC_RELOCATE 0
#define R3DGS_MCMC_GROW 1

/* How r3dgs_mcmc_move fills the rows of one tensor (the struct has the shape of r3dgs_densify_tensor). */
#define R3DGS_MCMC_COPY 0     /* a relocated / new row is its source's row; every other row stays (a parameter, _degrees) */
#define R3DGS_MCMC_MOMENT 1   /* exp_avg, exp_avg_sq.  RELOCATE: zero at the drawn sources; a relocated row keeps its own unless
                                 zero_relocated.  GROW: old rows keep theirs, new rows are zero */
#define R3DGS_MCMC_OPACITY 2  /* as COPY, and a drawn source takes its new raw opacity first; 1 word per row */
#define R3DGS_MCMC_SCALING 3  /* as COPY, and a drawn source takes its new raw scaling first; 3 words per row */

typedef struct {
    const void* src; /* [P, row_words] 4-byte elements */
    void* dst;       /* RELOCATE: == src (in place); GROW: [P + n_new, row_words] */
    int row_words;   /* 4-byte words per row; 0: the tensor has no columns and is skipped */
    int kind;        /* R3DGS_MCMC_* */
} r3dgs_mcmc_tensor;

/* Bytes of device scratch that plan and move share for P Gaussians and up to n_draws draws; 0 for P <= 0.  A pure function of
 * its arguments. */
size_t r3dgs_mcmc_workspace_bytes(int P, int n_draws);

/* xyz [P,3] is updated in place; opacity_raw [P], scaling_raw [P,3], rotation_raw [P,4] (16-byte aligned), noise [P,3]
 * standard normal.  scale = noise_lr * the current learning rate of xyz.  One launch; capturable in a graph. */
int r3dgs_mcmc_noise(int P, float* xyz, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
                     const float* noise, float scale, void* stream);

/* uniforms: fp32 in [0,1), P entries (RELOCATE) or n_draws entries (GROW).  sampled: int32, P entries (RELOCATE) or n_draws
 * (GROW).  slots: int32 [P], RELOCATE only (may be NULL for GROW).  ratio: int32 [P].  totals: int32 [8] on the device.
 * workspace: r3dgs_mcmc_workspace_bytes(P, n_draws) bytes, 16-byte aligned, not cleared.  n_draws is ignored for RELOCATE. */
int r3dgs_mcmc_plan(int P, const float* opacity_raw, float min_opacity, int mode, int n_draws, const float* uniforms,
                    int* sampled, int* slots, int* ratio, int* totals, char* workspace, void* stream);

/* Writes the n tensors of the table from a plan's sampled / slots / ratio / totals.  opacity_raw [P], scaling_raw [P,3]: the
 * source parameters (in RELOCATE the same memory as the table's OPACITY and SCALING entries: the new values are computed
 * into the workspace by a launch of their own before any row is written).  n_new: rows appended (GROW; 0 for RELOCATE, whose
 * number of relocated rows is totals[1], read on the device).  zero_relocated: RELOCATE, also zero the moments of the
 * relocated rows.  No host wait; with RELOCATE no size changes and the call is capturable in a graph. */
int r3dgs_mcmc_move(int P, int mode, int n_new, int zero_relocated, float min_opacity, int n, const r3dgs_mcmc_tensor* tensors,
                    const float* opacity_raw, const float* scaling_raw, const int* sampled, const int* slots, const int* ratio,
                    const int* totals, char* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_MCMC_H */
