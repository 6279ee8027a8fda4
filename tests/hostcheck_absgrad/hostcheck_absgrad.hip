// hostcheck_absgrad.hip -- the abs accumulate of the backward blend (csrc/blend_math.h bwd_accumulate_abs / splat_abs_grad_of)
// run on the CPU over the oracle's lists, with the kernel's own bookkeeping: per (tile, entry) the moments and the two abs sums
// are added over the tile's pixels in float, turned into gradients once per (tile, entry) (splat_grad_of, splat_abs_grad_of,
// the viewport factors), and those rows are added per Gaussian.  Built by tests/hostcheck_build.py; tests/test_absgrad_cpu.py
// holds the result to the float64 restatement tests/absgrad_ref.py.
#include <vector>

#include "../../reduced-3dgs_amd/csrc/blend_math.h"

using namespace r3;

namespace {
constexpr int kTile = 16;
Splat splat_of(const float* xy, const float* conic_op, const float* rgb, unsigned id)
{
    Splat s;
    s.x = xy[2 * id];
    s.y = xy[2 * id + 1];
    s.cA = conic_op[4 * id];
    s.cB = conic_op[4 * id + 1];
    s.cC = conic_op[4 * id + 2];
    s.op = conic_op[4 * id + 3];
    s.r = rgb[3 * id];
    s.g = rgb[3 * id + 1];
    s.b = rgb[3 * id + 2];
    return s;
}
}  // namespace

extern "C" {

// signed_out, abs_out: double [P][2], zeroed by the caller
void hc_absgrad(int P, int W, int H, const unsigned* ranges, const unsigned* point_list, const float* bg, const float* xy,
                const float* conic_op, const float* rgb, const float* final_T, const unsigned* n_contrib, const float* dL_dpix,
                double* signed_out, double* abs_out)
{
    (void)P;
    const int gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    const size_t plane = (size_t)W * H;
    const float half_w = 0.5f * (float)W, half_h = 0.5f * (float)H;
    for (int tile = 0; tile < gx * gy; tile++) {
        const unsigned r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        std::vector<SplatSums> sums(r1 - r0);
        std::vector<SplatAbsSums> asums(r1 - r0);
        std::vector<char> hit(r1 - r0, 0);
        for (auto& u : sums) u.sx = u.sy = u.sxx = u.sxy = u.syy = u.sm = u.r = u.g = u.b = 0.f;
        for (auto& u : asums) u.ax = u.ay = 0.f;
        for (int py = (tile / gx) * kTile; py < H && py < (tile / gx + 1) * kTile; py++)
            for (int px = (tile % gx) * kTile; px < W && px < (tile % gx + 1) * kTile; px++) {
                const size_t pix = (size_t)W * py + px;
                BwdPix p;
                const float g0 = dL_dpix[pix], g1 = dL_dpix[plane + pix], g2 = dL_dpix[2 * plane + pix];
                bwd_pix_init(p, final_T[pix], n_contrib[pix], g0, g1, g2, bg[0] * g0 + bg[1] * g1 + bg[2] * g2);
                for (long pos = (long)p.last - 1; pos >= 0; pos--) {
                    const QSplat s = scale_splat(splat_of(xy, conic_op, rgb, point_list[r0 + pos]));
                    BwdEval e;
                    if (!bwd_test(s, (float)px, (float)py, (unsigned)pos, p, e)) continue;
                    bwd_accumulate_abs(s, e, p, asums[pos]);   // in front of bwd_accumulate: it reads the state that advances
                    bwd_accumulate(s, e, p, sums[pos]);
                    hit[pos] = 1;
                }
            }
        for (unsigned k = 0; k < r1 - r0; k++) {
            if (!hit[k]) continue;
            const unsigned id = point_list[r0 + k];
            const QSplat s = scale_splat(splat_of(xy, conic_op, rgb, id));
            const SplatGrad g = splat_grad_of(s, sums[k]);
            float ax, ay;
            splat_abs_grad_of(s, asums[k], &ax, &ay);
            signed_out[2 * (size_t)id] += (double)(g.mx * half_w);
            signed_out[2 * (size_t)id + 1] += (double)(g.my * half_h);
            abs_out[2 * (size_t)id] += (double)(ax * half_w);
            abs_out[2 * (size_t)id + 1] += (double)(ay * half_h);
        }
    }
}

}  // extern "C"
