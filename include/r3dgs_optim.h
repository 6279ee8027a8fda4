/* r3dgs_optim.h -- C ABI of the fused Adam step (reduced-3dgs_amd/csrc/optim.hip), the optimizer of
 * scene/gaussian_model.py:217 (torch.optim.Adam(l, lr=0.0, eps=1e-15), six parameter groups) in one launch per step
 * instead of torch's ~8 elementwise passes per group.  The Python surface is r3dgs_optim.Adam.
 * Same conventions as r3dgs_rasterizer.h: device pointers, fp32; `void* stream` is a hipStream_t; return >= 0 on success,
 * < 0 with the message in r3dgs_last_error().  No call synchronises the host, allocates or uses atomics: results are
 * identical run to run, and r3dgs_adam_step_capturable can be captured in a graph.
 *
 * Each segment is one parameter tensor of n contiguous floats; the four arrays of a segment must not overlap each other
 * or another segment's.  Any float alignment is accepted (gradients may be views at odd offsets into one flat buffer):
 * a segment whose four pointers share their 16-byte phase runs 16-byte loads and stores, any other runs 4-byte ones.
 * Up to R3DGS_ADAM_MAX_SEGMENTS segments go into one launch (by value, in the kernel arguments); more take more launches. */
#ifndef R3DGS_OPTIM_H
#define R3DGS_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R3DGS_ADAM_MAX_SEGMENTS 32

/* One tensor of a step, with the fp32 scalars of its group, each a double rounded to fp32 once (adam_math.h):
 *   lerp_weight = 1 - beta1,  beta2,  addcmul_value = 1 - beta2,  bc2_sqrt = (1 - beta2**step) ** 0.5,  eps,
 *   step_size = -(lr / (1 - beta1**step)),  step being the count after this step's bump. */
typedef struct r3dgs_adam_segment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;
    float lerp_weight;
    float beta2;
    float addcmul_value;
    float bc2_sqrt;
    float eps;
    float step_size;
} r3dgs_adam_segment;

/* One Adam step of n_segments tensors (segments: a host array), torch.optim.Adam's default step bit for bit. */
int r3dgs_adam_step(int n_segments, const r3dgs_adam_segment* segments, void* stream);

/* A segment of the capturable step: the step count and optionally lr live on the device, so a captured graph reads them at
 * replay.  The kernel uses step[0] + 1 and then stores it back into step[0] (a second, one-thread-per-segment launch);
 * lr is lr[0] when lr is not NULL, else lr_value.  The bias corrections are computed per workgroup in double from the
 * device step, then rounded to fp32 as in r3dgs_adam_segment (not bit-identical to torch's capturable arithmetic). */
typedef struct r3dgs_adam_capturable_segment {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    const float* lr;
    long long n;
    double lr_value;
    double beta1;
    double beta2;
    double eps;
} r3dgs_adam_capturable_segment;

int r3dgs_adam_step_capturable(int n_segments, const r3dgs_adam_capturable_segment* segments, void* stream);

/* The visibility-gated step (opt-in; the two calls above are unchanged by it).  Every segment is a [P, row_len[i]] array
 * (n == P * row_len[i]; row_len: a host array of n_segments ints >= 1) and radii is the rasterizer's device int[P].
 * Gaussian j is visible iff radii[j] > 0.  The elements of a visible Gaussian take exactly the step of the dense call with
 * the same scalars; those of any other keep the bits of param, exp_avg and exp_avg_sq, and their gradient is not looked at
 * (it may hold NaN or Inf).  The step count and so the bias corrections are the tensor's, not the row's, as in
 * torch.optim.SparseAdam; with every Gaussian visible the result equals the dense call's bit for bit.  Unlike the dense
 * step, a culled Gaussian's moments do not decay and its parameters do not move on their momentum.
 * Refused before anything is launched: row_len[i] < 1, n != P * row_len[i], radii NULL with P > 0, and all the dense calls
 * refuse.  P == 0 launches no step kernel (the capturable form still bumps the counts).  radii is read on the stream at
 * run time, so a captured graph follows new contents of the same buffer. */
int r3dgs_adam_step_visible(int n_segments, const r3dgs_adam_segment* segments, const int* row_len, const int* radii,
                            long long P, void* stream);
int r3dgs_adam_step_capturable_visible(int n_segments, const r3dgs_adam_capturable_segment* segments, const int* row_len,
                                       const int* radii, long long P, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R3DGS_OPTIM_H */
