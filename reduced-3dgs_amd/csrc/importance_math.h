// importance_math.h -- arithmetic of the per-Gaussian blend-contribution scores (importance.hip, include/r3dgs_importance.h):
// the blend weight w = alpha * T_before of a list entry at a pixel, the 16-byte row a wave leaves per (list slot, quadrant),
// and the per-Gaussian fold of those rows into the caller's buffers.
//
// __host__ __device__ like blend_math.h / aux_math.h / feature_math.h, so that tests/hostcheck_importance/
// hostcheck_importance.hip runs the very same steps on the CPU.
//
// The step IS the forward's step (fwd_alpha / fwd_apply) on a splat without colour: T, Tf and last come out of fwd_apply
// itself, bit for bit, and w is the product fwd_apply forms for its colour channels (one rounding).  T runs forward from 1:
// nothing is recovered by division.
#pragma once
#include "blend_math.h"

namespace r3 {

constexpr int kImpQuads = 4;   // rows per pair: one per 8x8 quadrant of the tile, in quadrant order

// the list entry as the forward's step takes it, without colour
R3_HD QSplat imp_splat(float x, float y, float qa, float qb, float qc, float op)
{
    QSplat s;
    s.x = x;
    s.y = y;
    s.qa = qa;
    s.qb = qb;
    s.qc = qc;
    s.op = op;
    s.r = s.g = s.b = 0.f;
    return s;
}

// One list entry (1-based position `pos1`) against one pixel of weight `m`, whose forward blended `n` entries deep.  True
// when the pixel blends the entry AND counts (m != 0; either zero masks the pixel out); then *w = alpha * T_before and
// *mw = m * w, otherwise both are 0.  The pixel's T moves whether it counts or not.
R3_HD bool imp_step(const QSplat& s, float pxf, float pyf, uint32_t pos1, uint32_t n, float m, FwdPix& p, float* w, float* mw)
{
    bool in_bound;
    const float alpha = fwd_alpha(s, pxf, pyf, &in_bound);
    float T_before;
    const int r = fwd_apply(s, alpha, in_bound && pos1 <= n, pos1, p, &T_before);
    const bool hit = r == 1 && m != 0.0f;
    const float wk = alpha * T_before;
    *w = hit ? wk : 0.f;
    *mw = hit ? m * wk : 0.f;
    return hit;
}

// 16 B: what a wave leaves per (list slot, quadrant)
struct ImpRow {
    float sum;        // sum over the quadrant's counted pixels of m * w, in the order of imp_tree_sum
    float max;        // the largest w among them
    uint32_t count;   // how many they are
    uint32_t zero;
};

// The order of the wave's reductions (importance.hip wave_sum / wave_max: lane ^ 1, lane ^ 2, the mirror of a half row, the
// mirror of a row, lane ^ 16, lane ^ 32 -- at every step both partners combine the same two numbers, so every lane holds
// the same bits): a balanced tree over neighbouring lanes.  v: the 64 lanes' values, overwritten.
inline float imp_tree_sum(float* v)
{
    for (int n = 64; n > 1; n >>= 1)
        for (int i = 0; i < n / 2; i++) v[i] = v[2 * i] + v[2 * i + 1];
    return v[0];
}

inline float imp_tree_max(float* v)
{
    for (int n = 64; n > 1; n >>= 1)
        for (int i = 0; i < n / 2; i++) v[i] = fmaxf(v[2 * i], v[2 * i + 1]);
    return v[0];
}

// ---- the per-Gaussian fold ------------------------------------------------------------------------------------------
struct ImpScore {
    double sum;
    float max;
    long long count;
    int views;
};

R3_HD void imp_score_clear(ImpScore& a)
{
    a.sum = 0.0;
    a.max = 0.f;
    a.count = 0;
    a.views = 0;
}

// a row of the Gaussian's run, in sorted order (list slot ascending, quadrant 0..3)
R3_HD void imp_add_row(ImpScore& a, float sum, float max, uint32_t count)
{
    a.sum += (double)sum;
    a.max = fmaxf(a.max, max);
    a.count += (long long)count;
}

// The overflow rule: a Gaussian whose run of pairs is shorter than the pairs the forward wanted for it (tiles_touched) lost
// some to an overflowed reservation and contributes nothing for the view.
R3_HD bool imp_run_complete(uint32_t run, uint32_t tiles_touched) { return run == tiles_touched; }

// What the caller's buffers hold after the view: `view` (its rows added by imp_add_row; views is not looked at) replaces
// `held`, or with `accumulate` is folded into it.
R3_HD ImpScore imp_fold(const ImpScore& view, bool complete, bool accumulate, const ImpScore& held)
{
    ImpScore v;
    imp_score_clear(v);
    if (complete) {
        v.sum = view.sum;
        v.max = view.max;
        v.count = view.count;
    }
    v.views = v.count > 0 ? 1 : 0;
    if (!accumulate) return v;
    ImpScore o;
    o.sum = held.sum + v.sum;
    o.max = fmaxf(held.max, v.max);
    o.count = held.count + v.count;
    o.views = held.views + v.views;
    return o;
}

}  // namespace r3
