// aux_math.h -- per-(pixel, Gaussian) arithmetic of the auxiliary maps (aux_maps.hip): expected depth, accumulated opacity
// and median depth, replayed from the state a forward pass left.
//
// __host__ __device__ like blend_math.h, so that tests/hostcheck_aux/hostcheck_aux.hip runs the very same step on the CPU.
//
// Definitions, per pixel, over the first n = n_contrib[pixel] entries of the tile's list (the forward's own count, so the
// stop is the forward's stop), with the forward's per-entry rule (fwd_alpha / fwd_apply: skip on power > 0 or
// alpha < 1/255, alpha = min(0.99, op * exp), T <- T - alpha T) and z_k the view depth of entry k:
//   depth        = sum over the blended entries of z_k * alpha_k * T_before_k   (fp32, list order; not normalised, no
//                  background term)
//   alpha        = 1 - final_T                                                   (from the forward's stored final_T)
//   median_depth = z_k of the first blended entry after which T < 0.5, 0 if there is none
//   n == 0: 0 in all three.
// The step below IS the forward's step with the colour triple replaced by (z, 0, 0): T, Tf and last come out of
// fwd_apply itself, so they are the forward's bit for bit, and the depth sum is accumulated exactly as a colour channel is.
// The maps carry no gradient.
#pragma once
#include "blend_math.h"

namespace r3 {

struct AuxPix {
    FwdPix f;         // the forward's per-pixel state; C0 is the depth sum (C1, C2 stay 0)
    float median;     // z of the first blended entry that left T < 0.5 (0: none so far)
    uint32_t cross;   // 1-based list position of that entry (0: none so far)
};

R3_HD void aux_pix_init(AuxPix& p, bool inside)
{
    fwd_pix_init(p.f, inside);
    p.median = 0.f;
    p.cross = 0u;
}

// the list entry as the forward's step takes it, with the view depth where the colour was
R3_HD QSplat aux_splat(float x, float y, float qa, float qb, float qc, float op, float z)
{
    QSplat s;
    s.x = x;
    s.y = y;
    s.qa = qa;
    s.qb = qb;
    s.qc = qc;
    s.op = op;
    s.r = z;
    s.g = 0.f;
    s.b = 0.f;
    return s;
}

// Blends an entry (s.r = its view depth) of opacity-weighted falloff `alpha` into pixel `p`, whose forward blended `n`
// entries deep: an entry behind position n is not looked at.  Returns fwd_apply's code (0: skipped, 1: blended, 2: saturated).
R3_HD int aux_apply(const QSplat& s, float alpha, bool in_bound, uint32_t pos1, uint32_t n, AuxPix& p)
{
    float T_before;
    const int r = fwd_apply(s, alpha, in_bound && pos1 <= n, pos1, p.f, &T_before);
    if (r == 1 && p.cross == 0u && p.f.Tf < 0.5f) {   // T only falls: the first crossing of 0.5 is latched
        p.cross = pos1;
        p.median = s.r;
    }
    return r;
}

// One list entry against one pixel.
R3_HD int aux_step(const QSplat& s, float pxf, float pyf, uint32_t pos1, uint32_t n, AuxPix& p)
{
    bool in_bound;
    const float alpha = fwd_alpha(s, pxf, pyf, &in_bound);
    return aux_apply(s, alpha, in_bound, pos1, n, p);
}

R3_HD int aux_step(const Splat& s, float z, float pxf, float pyf, uint32_t pos1, uint32_t n, AuxPix& p)
{
    const QSplat q = scale_splat(s);
    return aux_step(aux_splat(q.x, q.y, q.qa, q.qb, q.qc, q.op, z), pxf, pyf, pos1, n, p);
}

R3_HD float aux_depth(const AuxPix& p) { return p.f.C0; }

}  // namespace r3
