// densify_math.h -- per-Gaussian arithmetic of densification (densify.hip): the decision flags of clone / split / prune and the
// rows of a split Gaussian's children.  Shared with the CPU test shim tests/hostcheck_densify/hostcheck_densify.hip so the
// exact source a lane executes is checked without a GPU.
//
// What it restates (scene/gaussian_model.py of the reference, restated line by line in tests/densify_ref.py):
//   :671-672  grads = xyz_gradient_accum / denom; NaN -> 0                                        densify_grad
//   :653-655  clone: grads >= max_grad and max(exp(_scaling)) <= percent_dense * extent          densify_flags
//   :626-630  split: grads >= max_grad and max(exp(_scaling)) >  percent_dense * extent          densify_flags
//   :685-689  prune: sigmoid(_opacity) < min_opacity [or max_radii2D > max_screen_size or max scale > 0.1 extent]
//   :636-637  xyz_child = R(q) (noise * scale) + xyz                                              child_xyz
//   :638      scaling_child = log(scale / (0.8 N)), N = 2                                         child_scaling
// The activations are the ones the rest of the library uses: stats_sigmoid (stats_math.h), scale_act and quat_act
// (param_math.h).  quat_act divides by the correctly rounded norm (and by 1e-12 for a zero quaternion), where the reference's
// build_rotation divides by an fp32 chain of four roundings (and by zero): the children of one parent differ from the
// reference's in the last bits of R, by less than the bound tests/densify_ref.py derives.
// densify.hip is compiled with -ffp-contract=off and correctly rounded fp32 divide and sqrt (build.py EXACT): every operation
// written here is one fp32 rounding, in the order written; expf and logf are the only ones that are not bit-reproducible
// between host and device (<= 1 ulp each).
#ifndef R3DGS_DENSIFY_MATH_H
#define R3DGS_DENSIFY_MATH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "param_math.h"
#include "stats_math.h"

namespace r3 {

constexpr int kSplitChildren = 2;        // N of densify_and_split (:622)
constexpr float kChildShrink = 1.6f;     // 0.8 * N as a Python double, rounded to fp32 once where torch divides by it (:638)

// One byte per source Gaussian.
constexpr uint8_t kFlagClone = 1;        // appended once more, as it is (:659-665)
constexpr uint8_t kFlagSplit = 2;        // replaced by its two children (:633-648)
constexpr uint8_t kFlagPrunedSelf = 4;   // the prune mask of the row itself -- and of its clone, which is the same row
constexpr uint8_t kFlagPrunedChild = 8;  // the prune mask of its children (both have the same opacity and scaling)

// The host's thresholds, each computed as a Python double and rounded to fp32 once.
struct DensifyThresholds {
    float max_grad;       // clone / split: grads >= max_grad
    float dense_scale;    // percent_dense * extent
    float min_opacity;
    float max_screen;     // max_screen_size (read only when `screen`)
    float world_scale;    // 0.1 * extent    (read only when `screen`)
    int densify;          // 1: densify_and_prune; 0: prune() on its own (nothing is cloned or split)
    int screen;           // max_screen_size is truthy: the two size terms of the prune mask act
};

// :671-672.  One correctly rounded divide; 0 / 0 = NaN becomes 0, x / 0 = inf stays (and passes every threshold).
__host__ __device__ inline float densify_grad(float accum, float denom)
{
    const float g = accum / denom;
    return g != g ? 0.f : g;
}

__host__ __device__ inline float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// :638.  Roundings: the divide, logf (<= 1 ulp).
__host__ __device__ inline float child_scaling(float scale) { return logf(scale / kChildShrink); }

// The flag byte of one source Gaussian.  max_radii is max_radii2D[i]; inside densify_and_prune densification_postfix
// (:617-620) has zeroed it before prune() looks, so the screen-size term compares 0 with the threshold there.
// The child's world-size term looks at exp(scaling_child), the activation of what was stored, not at scale / 1.6.
__host__ __device__ inline uint8_t densify_flags(const DensifyThresholds& t, float accum, float denom, const float raw_scale[3],
                                                 float raw_opacity, float max_radii)
{
    const float s0 = scale_act(raw_scale[0]), s1 = scale_act(raw_scale[1]), s2 = scale_act(raw_scale[2]);
    const float smax = max3(s0, s1, s2);
    uint8_t f = 0;
    if (t.densify && densify_grad(accum, denom) >= t.max_grad) f |= smax <= t.dense_scale ? kFlagClone : kFlagSplit;
    const bool low = stats_sigmoid(raw_opacity) < t.min_opacity;
    const float radii = t.densify ? 0.f : max_radii;
    if (low || (t.screen && (radii > t.max_screen || smax > t.world_scale))) f |= kFlagPrunedSelf;
    if (f & kFlagSplit) {
        const float cmax = max3(scale_act(child_scaling(s0)), scale_act(child_scaling(s1)), scale_act(child_scaling(s2)));
        if (low || (t.screen && (0.f > t.max_screen || cmax > t.world_scale))) f |= kFlagPrunedChild;
    }
    return f;
}

// Row `row` of build_rotation(q) (utils/general_utils.py:78-99) for the normalised quaternion q = (r, x, y, z).
// Roundings per entry: the products, their sum or difference, the doubling (exact), the subtraction from 1.
__host__ __device__ inline void rotation_row(const float q[4], int row, float R[3])
{
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    if (row == 0) {
        R[0] = 1.f - 2.f * (y * y + z * z);
        R[1] = 2.f * (x * y - r * z);
        R[2] = 2.f * (x * z + r * y);
    } else if (row == 1) {
        R[0] = 2.f * (x * y + r * z);
        R[1] = 1.f - 2.f * (x * x + z * z);
        R[2] = 2.f * (y * z - r * x);
    } else {
        R[0] = 2.f * (x * z - r * y);
        R[1] = 2.f * (y * z + r * x);
        R[2] = 1.f - 2.f * (x * x + y * y);
    }
}

// Component `row` of a child's position (:635-637): sample = noise * scale (torch.normal(0, s) is randn * s), then
// (R[row,0] sample0 + R[row,1] sample1) + R[row,2] sample2, then + xyz -- in THIS order, no fma.
// scale: the parent's activated scale, scale_act(raw_scale[k]).
__host__ __device__ inline float child_xyz(int row, const float raw_q[4], const float scale[3], const float noise[3], float xyz)
{
    float q[4], R[3];
    quat_act(raw_q, q);
    rotation_row(q, row, R);
    const float a0 = noise[0] * scale[0], a1 = noise[1] * scale[1], a2 = noise[2] * scale[2];
    return ((R[0] * a0 + R[1] * a1) + R[2] * a2) + xyz;
}

}  // namespace r3

#endif  // R3DGS_DENSIFY_MATH_H
