// feature_math.h -- per-(pixel, Gaussian) arithmetic of the feature maps (feature_maps.hip, include/r3dgs_features.h): a
// per-Gaussian feature vector blended into a [C, H, W] map, replayed from the state a forward pass left, and the gradients
// through it.
//
// __host__ __device__ like blend_math.h / aux_math.h, so that tests/hostcheck_features/hostcheck_features.hip runs the very
// same steps on the CPU.  Channels are handled NC at a time (a register-resident group): every function below is a template
// on NC and sees one group's slice of the feature row.
//
// Forward: the step IS the forward's step (fwd_alpha / fwd_apply) on a splat without colour -- T, Tf and last come out of
// fwd_apply itself, bit for bit -- and each channel adds f_c * w with w = alpha * T_before, the product fwd_apply itself forms
// for its colour channels (one rounding), so a channel is accumulated exactly as a colour channel is.
//
// Backward: the colour backward's step (bwd_test, then the body of bwd_accumulate) with the colour triple replaced by the NC
// channels of the group and no background term:
//   d out_c / d f_kc    = alpha_k T_k                                   -> the channel sums
//   d out_c / d alpha_k = f_kc T_k - (sum_{j > k} f_jc alpha_j T_j) / (1 - alpha_k)
// A = sum_c g_c (the blend behind the entry), carried as the colour backward carries it.  The recurrence is linear in the
// channels, so a pixel may run one recurrence per group and the six geometric sums of the groups add up to the whole.
#pragma once
#include "aux_math.h"

namespace r3 {

constexpr int kFeatGroup = 16;   // the widest register-resident channel group; 4 and 8 serve small C

R3_HD QSplat feat_splat(float x, float y, float qa, float qb, float qc, float op)
{
    return aux_splat(x, y, qa, qb, qc, op, 0.f);
}

// ---- forward --------------------------------------------------------------------------------------------------------
template <int NC>
struct FeatPix {
    FwdPix f;        // the forward's per-pixel state (its colour sums stay 0)
    float acc[NC];   // the group's channel sums
};

template <int NC>
R3_HD void feat_pix_init(FeatPix<NC>& p, bool inside)
{
    fwd_pix_init(p.f, inside);
#pragma unroll
    for (int c = 0; c < NC; c++) p.acc[c] = 0.f;
}

// Blends an entry of opacity-weighted falloff `alpha` and feature slice `feat` into pixel `p`, whose forward blended `n`
// entries deep.  Returns fwd_apply's code (0: skipped, 1: blended, 2: saturated).
template <int NC>
R3_HD int feat_apply(const QSplat& s, float alpha, bool in_bound, uint32_t pos1, uint32_t n, const float* feat, FeatPix<NC>& p)
{
    float T_before;
    const int r = fwd_apply(s, alpha, in_bound && pos1 <= n, pos1, p.f, &T_before);
    if (r == 1) {
        const float w = alpha * T_before;
#pragma unroll
        for (int c = 0; c < NC; c++) p.acc[c] += feat[c] * w;
    }
    return r;
}

template <int NC>
R3_HD int feat_step(const QSplat& s, float pxf, float pyf, uint32_t pos1, uint32_t n, const float* feat, FeatPix<NC>& p)
{
    bool in_bound;
    const float alpha = fwd_alpha(s, pxf, pyf, &in_bound);
    return feat_apply<NC>(s, alpha, in_bound, pos1, n, feat, p);
}

// ---- backward -------------------------------------------------------------------------------------------------------
template <int NC>
struct FeatBwdPix {
    BwdPix b;      // T, A and last as the colour backward keeps them (its g0..g2 stay 0)
    float g[NC];   // dL_dout of the group's channels at this pixel
};

template <int NC>
R3_HD void feat_bwd_pix_init(FeatBwdPix<NC>& p, bool inside, float T_final, uint32_t n_contrib, const float* g)
{
    bwd_pix_init(p.b, T_final, inside ? n_contrib : 0u, 0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < NC; c++) p.g[c] = g[c];
}

// what a lane accumulates per list entry: the six geometric moments (SplatSums, its colour sums unused) and the channel sums
template <int NC>
struct FeatSums {
    SplatSums s;
    float f[NC];
};

template <int NC>
R3_HD void feat_sums_clear(FeatSums<NC>& a)
{
    aux_sums_clear(a.s);
#pragma unroll
    for (int c = 0; c < NC; c++) a.f[c] = 0.f;
}

// An entry that passed bwd_test against pixel p: bwd_accumulate's body over NC channels.  GEOM = false leaves the geometric
// moments alone (frozen geometry: only T is carried).
template <int NC, bool GEOM>
R3_HD void feat_bwd_apply(const BwdEval& e, const float* feat, FeatBwdPix<NC>& p, FeatSums<NC>& a)
{
    const float ra = R3_RCP(1.0f - e.alpha);
    p.b.T = p.b.T * ra;   // T recovered by division (backward.cu:541)
    const float dch = e.alpha * p.b.T;
#pragma unroll
    for (int c = 0; c < NC; c++) a.f[c] += dch * p.g[c];
    if (GEOM) {
        float cg = 0.f;
#pragma unroll
        for (int c = 0; c < NC; c++) cg += feat[c] * p.g[c];
        const float behind = cg - p.b.A;
        const float dL_dalpha = behind * p.b.T;
        p.b.A = fmaf(e.alpha, behind, p.b.A);
        const float m = e.G * dL_dalpha;
        a.s.sm += m;
        a.s.sx = fmaf(m, e.o.dx, a.s.sx);
        a.s.sy = fmaf(m, e.o.dy, a.s.sy);
        a.s.sxx = fmaf(m, e.o.dxx, a.s.sxx);
        a.s.sxy = fmaf(m, e.o.dxy, a.s.sxy);
        a.s.syy = fmaf(m, e.o.dyy, a.s.syy);
    }
}

// One list entry (0-based position `pos`) against one pixel; true when the entry contributed.
template <int NC, bool GEOM>
R3_HD bool feat_bwd_step(const QSplat& s, float pxf, float pyf, uint32_t pos, const float* feat, FeatBwdPix<NC>& p,
                         FeatSums<NC>& a)
{
    BwdEval e;
    if (!bwd_test(s, pxf, pyf, pos, p.b, e)) return false;
    feat_bwd_apply<NC, GEOM>(e, feat, p, a);
    return true;
}

}  // namespace r3
