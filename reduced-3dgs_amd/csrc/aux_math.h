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
// The maps themselves are plain arrays; the second half of this file carries gradients through them.
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

// ---------------------------------------------------------------------------------------------------------------------
// Gradients THROUGH the maps (aux_bwd.hip, include/r3dgs_aux.h r3dgs_aux_maps_backward).
//
// depth = sum z alpha T is a colour channel whose colour is z, alpha = 1 - T_final a colour channel whose colour is 1 over a
// zero background: with upstream gradients (g_D, g_A, g_M) of the three maps, the per-(pixel, entry) step is the colour
// backward's own (blend_math.h bwd_test / bwd_accumulate) on a splat of colour (z, 1, 0) and a pixel gradient (g_D, g_A, 0)
// without a background term:
//   d depth / d z_k     = alpha_k T_k                                                   -> SplatSums::r, the z sum
//   d depth / d alpha_k = z_k T_k - (sum_{j > k} z_j alpha_j T_j) / (1 - alpha_k)
//   d alpha / d alpha_k = T_k - (sum_{j > k} alpha_j T_j) / (1 - alpha_k) = T_final / (1 - alpha_k)
// (SplatSums::g collects d/d(the colour 1): nobody reads it.)  The median depth hands g_M to the z of the entry it selected and
// to nothing else: walking back to front with T recovered by division, that is the one blended entry with T behind it < 0.5
// and T in front of it >= 0.5 (the recovered T only grows towards the front, so exactly one entry qualifies when
// T_final < 0.5 and none otherwise; where the forward's T came within an ulp of 0.5 the neighbour may be chosen instead --
// the pixels tests/aux_ref.py flags as median_ambig).
// ---------------------------------------------------------------------------------------------------------------------
#include "gauss_math.h"

namespace r3 {

constexpr int kAuxSums = 7;        // per (pair, quadrant): sx, sy, sxx, sxy, syy, sm, sz
constexpr int kAuxRowFloats = 8;   // 32-byte rows of the workspace slab (the eighth float is 0)
constexpr int kAuxQuads = 4;       // rows per pair: one per 8x8 quadrant of the tile, in quadrant order

R3_HD QSplat aux_bwd_splat(float x, float y, float qa, float qb, float qc, float op, float z)
{
    QSplat s = aux_splat(x, y, qa, qb, qc, op, z);
    s.g = 1.f;
    return s;
}

// a pixel in front of its back-to-front walk: the forward's final T and last contributor (0 outside the image: no entry is
// in its list), the gradients of depth and alpha where the colour backward has dL_dpixel, no background term
R3_HD void aux_bwd_pix_init(BwdPix& p, bool inside, float T_final, uint32_t n_contrib, float g_depth, float g_alpha)
{
    bwd_pix_init(p, T_final, inside ? n_contrib : 0u, g_depth, g_alpha, 0.f, 0.f);
}

R3_HD void aux_sums_clear(SplatSums& a) { a.sx = a.sy = a.sxx = a.sxy = a.syy = a.sm = a.r = a.g = a.b = 0.f; }

// An entry that passed bwd_test against pixel p: the colour backward's step, and g_M into the z sum of the median's entry.
R3_HD void aux_bwd_apply(const QSplat& s, const BwdEval& e, BwdPix& p, float g_median, SplatSums& a)
{
    const float T_behind = p.T;
    bwd_accumulate(s, e, p, a);
    if (T_behind < 0.5f && !(p.T < 0.5f)) a.r += g_median;
}

// One list entry (0-based position `pos`) against one pixel; true when the entry contributed.
R3_HD bool aux_bwd_step(const QSplat& s, float pxf, float pyf, uint32_t pos, BwdPix& p, float g_median, SplatSums& a)
{
    BwdEval e;
    if (!bwd_test(s, pxf, pyf, pos, p, e)) return false;
    aux_bwd_apply(s, e, p, g_median, a);
    return true;
}

R3_HD void aux_row_of(const SplatSums& a, float* row)   // the seven sums in the slab's order
{
    row[0] = a.sx;
    row[1] = a.sy;
    row[2] = a.sxx;
    row[3] = a.sxy;
    row[4] = a.syy;
    row[5] = a.sm;
    row[6] = a.r;
}

// What the maps' gradients leave per Gaussian.
struct AuxGaussGrad {
    float mean2D[2];   // view-space gradient of the pixel mean (with the 0.5 W / 0.5 H viewport factors: what densification reads)
    float mean3D[3];
    float opacity;     // of the RAW opacity
    float scale[3], rot[4], cov6[6];
};

// The per-Gaussian chain behind the summed rows (`sums`: the seven sums of a Gaussian over all its pairs and quadrants, in
// double): moments -> splat gradients (splat_grad_of, on the record's conic scaled as QSplat has it), then the colour
// backward's chain -- cov2d_backward, project_backward, the z term through the third row of the view transform (the layout
// xform4x3 reads), cov3d_backward, opacity_backward.  F64: the _f64 forms, as preprocess_bwd selects them.
// `rec6`: x, y, conic A, B, C and the activated opacity of the Gaussian's record.  cov3D_precomp != nullptr: the covariance
// was given (scale / rot stay 0, cov6 is the result); otherwise scales / rotations are the activated values.
// `screen` (optional): receives the screen-space gradients the chain starts from -- dL_dconic (A, B, C) as cov2d_backward is fed
// it and dL/dz of the view depth alone -- for a camera pass behind this one (camera_math.h camera_maps_gaussian).
struct AuxScreenGrad {
    float conic[3];   // A, B, C
    float z;
};

template <bool F64>
R3_HD void aux_bwd_chain(const Camera& cam, const float* rec6, const double* sums, const float* mean3, const float* scales,
                         const float* rotations, const float* cov3D_precomp, AuxGaussGrad& o, AuxScreenGrad* screen = nullptr)
{
    Splat sp;
    sp.x = rec6[0];
    sp.y = rec6[1];
    sp.cA = rec6[2];
    sp.cB = rec6[3];
    sp.cC = rec6[4];
    sp.op = rec6[5];
    sp.r = sp.g = sp.b = 0.f;
    SplatSums u;
    u.sx = (float)sums[0];
    u.sy = (float)sums[1];
    u.sxx = (float)sums[2];
    u.sxy = (float)sums[3];
    u.syy = (float)sums[4];
    u.sm = (float)sums[5];
    u.r = (float)sums[6];
    u.g = u.b = 0.f;
    const SplatGrad g = splat_grad_of(scale_splat(sp), u);
    o.mean2D[0] = g.mx * (0.5f * (float)cam.W);   // backward.cu:498-499
    o.mean2D[1] = g.my * (0.5f * (float)cam.H);
    if (screen) {
        screen->conic[0] = g.cA;
        screen->conic[1] = g.cB;
        screen->conic[2] = g.cC;
        screen->z = g.r;
    }
    float c6[6], sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f};
    if (cov3D_precomp) {
        for (int k = 0; k < 6; k++) c6[k] = cov3D_precomp[k];
    } else {
        for (int k = 0; k < 3; k++) sc[k] = scales[k];
        for (int k = 0; k < 4; k++) q[k] = rotations[k];
        cov3d_from_scale_rot(sc, cam.scale_modifier, q, c6);
    }
    double dcov6d[6];
    if (F64) {
        cov2d_backward_f64(cam, mean3[0], mean3[1], mean3[2], c6, g.cA, g.cB, g.cC, dcov6d, o.mean3D);
        for (int k = 0; k < 6; k++) o.cov6[k] = (float)dcov6d[k];
    } else {
        cov2d_backward(cam, mean3[0], mean3[1], mean3[2], c6, g.cA, g.cB, g.cC, o.cov6, o.mean3D);
    }
    project_backward(cam, mean3[0], mean3[1], mean3[2], o.mean2D[0], o.mean2D[1], o.mean3D);
    // z = view[2] x + view[6] y + view[10] z + view[14]
    o.mean3D[0] += cam.view[2] * g.r;
    o.mean3D[1] += cam.view[6] * g.r;
    o.mean3D[2] += cam.view[10] * g.r;
    for (int k = 0; k < 3; k++) o.scale[k] = 0.f;
    for (int k = 0; k < 4; k++) o.rot[k] = 0.f;
    if (!cov3D_precomp) {
        if (F64)
            cov3d_backward_f64(sc, cam.scale_modifier, q, dcov6d, o.scale, o.rot);
        else
            cov3d_backward(sc, cam.scale_modifier, q, o.cov6, o.scale, o.rot);
    }
    o.opacity = opacity_backward(g.op, sp.op);
}

}  // namespace r3
