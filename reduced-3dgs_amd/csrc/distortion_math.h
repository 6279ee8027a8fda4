// distortion_math.h -- per-(pixel, Gaussian) arithmetic of the depth-distortion map and of the gradients through it
// (distortion.hip, include/r3dgs_distortion.h): the squared form of the 2DGS regulariser.
//
// __host__ __device__ like blend_math.h / aux_math.h, so that tests/hostcheck_distortion runs the very same steps on the CPU.
//
// Per pixel, over the entries k the forward blended (its skip rule, its stop n_contrib, exactly as aux_math.h walks them), with
// the blend weight w_k = alpha_k T_before_k and the mapped depth m_k of entry k:
//   distortion = sum_k w_k (m_k^2 A_<k + D2_<k - 2 m_k D1_<k) = sum_{j<k} w_j w_k (m_k - m_j)^2
//   A_<k = sum_{j<k} w_j,  D1_<k = sum_{j<k} w_j m_j,  D2_<k = sum_{j<k} w_j m_j^2;  no background term, 0 where nothing blended.
// With the pixel's totals A = sum w (= 1 - final_T), S1 = sum w m, S2 = sum w m^2:
//   distortion       = A S2 - S1^2
//   d dist / d w_k   = A m_k^2 - 2 m_k S1 + S2 = sum_j w_j (m_k - m_j)^2        (c_k)
//   d dist / d m_k   = 2 w_k (A m_k - S1)
// w_k depends on the alphas in front of it as a colour channel's weight does, so dL/dalpha_k is the colour backward's step
// (blend_math.h bwd_accumulate) on a splat of colour c_k under the pixel gradient g over a black background, and the z sum takes
// g 2 w_k (A m_k - S1) dm/dz where aux_bwd_apply takes g alpha T.
//
// Cancellation.  Every expression above is a sum of squares written as a difference of products: all depths are carried
// RELATIVE to a reference m_ref (every expression is invariant under the shift), the mapped depth of the tile's first list
// entry -- a function of the forward's state alone, so forward and backward agree on it with nothing stored.  Terms then scale
// with the tile's depth range squared, which is the scale of the result.  The forward's four running sums are double (a pixel
// adds dozens of such terms, and the value bar is 1e-5 of the map's maximum); they are rounded to fp32 once, on the store.
//
// Depth mappings, by (near, far):
//   near = far = 0  : linear, m = z (the view-space depth), dm/dz = 1
//   0 < near < far  : 2DGS's, m = far / (far - near) (1 - near / z), dm/dz = far near / ((far - near) z^2);
//                     shifted: m - m_ref = far near / (far - near) (z - z_ref) / (z z_ref), formed without cancellation.
#pragma once
#include "aux_math.h"
#include "blend_math.h"
#include "gauss_math.h"

namespace r3 {

R3_HD bool depth_map_valid(float near, float far) { return (near == 0.f && far == 0.f) || (0.f < near && near < far); }

struct DepthMap {
    float k;       // far near / (far - near); 0: the linear mapping
    float z_ref;   // view depth of the reference entry
};

R3_HD DepthMap depth_map_of(float near, float far, float z_ref)
{
    DepthMap d;
    d.k = (near == 0.f && far == 0.f) ? 0.f : (float)((double)far * (double)near / ((double)far - (double)near));
    d.z_ref = z_ref;
    return d;
}

// mapped depth of view depth z, relative to the reference's
R3_HD float mapped_depth_shifted(const DepthMap& d, float z)
{
    const float dz = z - d.z_ref;
    return d.k == 0.f ? dz : d.k * dz / (z * d.z_ref);
}

R3_HD float mapped_depth_dz(const DepthMap& d, float z) { return d.k == 0.f ? 1.0f : d.k / (z * z); }

// ---- forward ------------------------------------------------------------------------------------------------------------
struct DistPix {
    FwdPix f;                // the forward's per-pixel state (its colour sums are not read)
    double A, D1, D2, dist;  // sum w, sum w m, sum w m^2 over the entries blended so far (m shifted), and the map's value
};

R3_HD void dist_pix_init(DistPix& p, bool inside)
{
    fwd_pix_init(p.f, inside);
    p.A = p.D1 = p.D2 = p.dist = 0.0;
}

// Blends an entry (s.r = its SHIFTED mapped depth) of opacity-weighted falloff `alpha` into pixel `p`, whose forward blended
// `n` entries deep.  Returns fwd_apply's code (0: skipped, 1: blended, 2: saturated).
R3_HD int dist_apply(const QSplat& s, float alpha, bool in_bound, uint32_t pos1, uint32_t n, DistPix& p)
{
    float T_before;
    const int r = fwd_apply(s, alpha, in_bound && pos1 <= n, pos1, p.f, &T_before);
    if (r == 1) {
        const double w = (double)(alpha * T_before), m = (double)s.r;
        const double wm = w * m, wmm = wm * m;
        p.dist += wmm * p.A + w * p.D2 - 2.0 * wm * p.D1;
        p.A += w;
        p.D1 += wm;
        p.D2 += wmm;
    }
    return r;
}

R3_HD int dist_step(const QSplat& s, float pxf, float pyf, uint32_t pos1, uint32_t n, DistPix& p)
{
    bool in_bound;
    const float alpha = fwd_alpha(s, pxf, pyf, &in_bound);
    return dist_apply(s, alpha, in_bound, pos1, n, p);
}

// One list entry of view depth z against one pixel.
R3_HD int dist_step(const Splat& s, float z, const DepthMap& d, float pxf, float pyf, uint32_t pos1, uint32_t n, DistPix& p)
{
    const QSplat q = scale_splat(s);
    return dist_step(aux_splat(q.x, q.y, q.qa, q.qb, q.qc, q.op, mapped_depth_shifted(d, z)), pxf, pyf, pos1, n, p);
}

R3_HD float dist_value(const DistPix& p) { return (float)p.dist; }
R3_HD float dist_moment1(const DistPix& p) { return (float)p.D1; }   // the saved pair: shifted S1, S2
R3_HD float dist_moment2(const DistPix& p) { return (float)p.D2; }

// ---- backward -----------------------------------------------------------------------------------------------------------
struct DistTotals {   // of one pixel: A = 1 - final_T, the saved shifted moments
    float A, S1, S2;
};

// a pixel in front of its back-to-front walk: the colour backward's state under the pixel gradient (g, 0, 0), no background
R3_HD void dist_bwd_pix_init(BwdPix& p, bool inside, float T_final, uint32_t n_contrib, float g)
{
    aux_bwd_pix_init(p, inside, T_final, n_contrib, g, 0.f);
}

// An entry (s.r = its SHIFTED mapped depth m, dmdz = dm/dz at its view depth) that passed bwd_test against pixel p: the colour
// backward's step on the colour c = A m^2 - 2 m S1 + S2; the z sum a.r takes g w 2 (A m - S1) dm/dz.
R3_HD void dist_bwd_apply(const QSplat& s, float dmdz, const BwdEval& e, BwdPix& p, const DistTotals& t, SplatSums& a)
{
    const float m = s.r;
    const float lin = fmaf(t.A, m, -t.S1);                        // A m - S1 = sum_j w_j (m - m_j)
    QSplat c = s;
    c.r = fmaf(fmaf(t.A, m, -2.0f * t.S1), m, t.S2);              // c_k
    c.g = c.b = 0.f;
    const float r_before = a.r;
    a.r = 0.f;
    bwd_accumulate(c, e, p, a);                                    // a.r = g w_k (the gradient of the colour: not wanted)
    a.r = fmaf(a.r, 2.0f * lin * dmdz, r_before);
}

// One list entry (0-based position `pos`) against one pixel; true when the entry contributed.
R3_HD bool dist_bwd_step(const QSplat& s, float dmdz, float pxf, float pyf, uint32_t pos, BwdPix& p, const DistTotals& t,
                         SplatSums& a)
{
    BwdEval e;
    if (!bwd_test(s, pxf, pyf, pos, p, e)) return false;
    dist_bwd_apply(s, dmdz, e, p, t, a);
    return true;
}

}  // namespace r3
