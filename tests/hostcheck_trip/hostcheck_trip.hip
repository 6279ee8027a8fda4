// hostcheck_trip.hip -- TEST SHIM for tests/test_blend_trip_forms.py: runs the per-lane functions of blend_math.h that make
// up one (entry, quadrant) trip of the blend kernels on the CPU and returns every result as raw bits.  The test builds
// it twice -- with -DR3_OLD_TRIP_FORMS (the forms before the trip was rewritten) and without -- both with FMA
// contraction on, as blend.hip is compiled, and compares the two outputs bit for bit.
#include <cstring>

#define R3_TRIP_FORMS_ON_HOST 1
#include "../../reduced-3dgs_amd/csrc/blend_math.h"

using namespace r3;

static uint32_t bits(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

extern "C" {

// in: n x 16 floats  x y qa qb qc op r g b px py T A g0 g1 g2 ; aux: n x 3 uint32  pos  last  sum_bits (initial value of all nine sums)
// out: n x 40 uint32
void trip_sweep(int n, const float* in, const uint32_t* aux, uint32_t* out)
{
    for (int k = 0; k < n; k++) {
        const float* v = in + 16 * k;
        uint32_t* o = out + 40 * k;
        QSplat s;
        s.x = v[0]; s.y = v[1]; s.qa = v[2]; s.qb = v[3]; s.qc = v[4]; s.op = v[5]; s.r = v[6]; s.g = v[7]; s.b = v[8];
        const float px = v[9], py = v[10];
        // forward
        bool inb;
        const float alpha = fwd_alpha(s, px, py, &inb);
        FwdPix f;
        fwd_pix_init(f, true);
        f.T = v[11];
        f.Tf = v[11];
        float Tb = -7.f;
        const int r = fwd_apply(s, alpha, inb, aux[3 * k] + 1u, f, &Tb);
        o[0] = bits(alpha); o[1] = inb; o[2] = (uint32_t)r; o[3] = bits(f.T); o[4] = bits(f.Tf); o[5] = bits(f.C0);
        o[6] = bits(f.C1); o[7] = bits(f.C2); o[8] = f.last; o[9] = bits(Tb); o[10] = fwd_pix_live(f);
        // backward
        BwdPix b;
        bwd_pix_init(b, v[11], aux[3 * k + 1], v[13], v[14], v[15], v[12]);
        BwdEval e;
        const bool valid = bwd_test(s, px, py, aux[3 * k], b, e);
        float z;
        std::memcpy(&z, &aux[3 * k + 2], 4);
        SplatSums u;
        u.sx = u.sy = u.sxx = u.sxy = u.syy = u.sm = u.r = u.g = u.b = z;
        if (valid) bwd_accumulate(s, e, b, u);
        const SplatGrad g = splat_grad_of(s, u);
        o[11] = valid; o[12] = e.in_list; o[13] = e.in_bound; o[14] = e.visible; o[15] = bits(e.G); o[16] = bits(e.alpha);
        o[17] = bits(b.T); o[18] = bits(b.A);
        const float us[9] = {u.sx, u.sy, u.sxx, u.sxy, u.syy, u.sm, u.r, u.g, u.b};
        const float gs[9] = {g.mx, g.my, g.cA, g.cB, g.cC, g.op, g.r, g.g, g.b};
        for (int c = 0; c < 9; c++) {
            o[19 + c] = bits(us[c]);
            o[28 + c] = bits(gs[c]);
        }
        o[37] = bits(e.o.dxx); o[38] = bits(e.o.dxy); o[39] = bits(e.o.dyy);
    }
}
}
