// Host check of the feature maps (reduced-3dgs_amd/csrc/feature_math.h): a stand-alone program that runs the shared forward
// and backward steps on the CPU over the scene in the text file named on its command line, channel group by channel group as
// the kernels do (groups of kFeatGroup), and
//   * forward, per pixel: T and last of the feature run equal those of a plain fwd_step colour run over the same list, bit
//     for bit; T lies within gamma(k) T and every channel's sum within gamma(2 k + 2) * sum |terms| of a double
//     restatement that takes each entry's alpha and decisions from the fp32 rule (k: blended entries; the bounds of
//     tests/hostcheck_aux, built like it with -DR3_TRIP_FORMS_ON_HOST so that T <- fma(-alpha, T, T) is the device's one
//     rounding; a term adds one for w = alpha T, one for f w, and the sum in list order at most k; the absolute sum because
//     features carry a sign);
//   * backward, per (list slot, channel): the sum over the tile's pixels of alpha T g within gamma(3 k + 2 + 64) * sum |terms|
//     of the restatement -- T recovered by division carries 3 roundings per step behind it (1 - alpha, its reciprocal, the
//     product; k: the deepest such walk), the term 2 more, and a quadrant's fp32 sum at most 64 additions (the quadrants are
//     added in double);
//   * prints one line per Gaussian for tests/test_feature_maps_cpu.py to hold against tests/feature_ref.py:
//       id  d/dmean.x d/dmean.y  d/dconicA d/dconicB d/dconicC  d/dopacity  d/dfeature[0..C-1]
//     (splat_grad_of over the six geometric sums, added per slot in fp32 and per Gaussian in double, as the device pass adds).
// Built once plainly and once with -fsanitize=address,undefined on the host side.
//
// Input, whitespace separated:  W H P R ntiles C, ranges[ntiles][2], point_list[R], per pixel (H*W): n_contrib final_T,
//   per Gaussian (P): x y conicA conicB conicC opacity, features[P][C], g[C][H*W].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../reduced-3dgs_amd/csrc/feature_math.h"

using namespace r3;

namespace {

constexpr int NC = kFeatGroup;

double gamma_of(int m) { return m * 0x1p-24 / (1.0 - m * 0x1p-24); }

uint32_t bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

bool read_floats(FILE* f, float* p, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (std::fscanf(f, "%f", p + k) != 1) return false;
    return true;
}

int fail(const char* what, long a, long b, double got, double want)
{
    std::printf("hostcheck_features: FAIL %s at (%ld, %ld): got %.9g, want %.9g\n", what, a, b, got, want);
    return 1;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: hostcheck_features scene.txt\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int W, H, P, R, ntiles, C;
    if (std::fscanf(f, "%d %d %d %d %d %d", &W, &H, &P, &R, &ntiles, &C) != 6 || W < 1 || H < 1 || P < 0 || R < 0 || C < 1 ||
        ntiles != ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile))
        return 2;
    const int gx = (W + kTile - 1) / kTile;
    const size_t N = (size_t)W * H;
    std::vector<uint32_t> ranges((size_t)ntiles * 2), list((size_t)R), ncon(N);
    std::vector<float> finalT(N), rec((size_t)P * 6), feat((size_t)P * C), g((size_t)C * N);
    for (uint32_t& v : ranges)
        if (std::fscanf(f, "%u", &v) != 1) return 2;
    for (uint32_t& v : list)
        if (std::fscanf(f, "%u", &v) != 1 || v >= (uint32_t)P) return 2;
    for (size_t k = 0; k < N; k++)
        if (std::fscanf(f, "%u %f", &ncon[k], &finalT[k]) != 2) return 2;
    if (!read_floats(f, rec.data(), rec.size()) || !read_floats(f, feat.data(), feat.size()) || !read_floats(f, g.data(), g.size()))
        return 2;
    std::fclose(f);
    for (int t = 0; t < ntiles; t++)
        if (ranges[2 * t + 1] < ranges[2 * t] || ranges[2 * t + 1] > (uint32_t)R) return 2;

    auto splat_of = [&](uint32_t id) {
        const float* r = &rec[(size_t)id * 6];
        Splat s{r[0], r[1], r[2], r[3], r[4], r[5], 0.f, 0.f, 0.f};
        return scale_splat(s);
    };
    const int groups = (C + NC - 1) / NC;
    auto slice = [&](const float* row, int c0, float* out) {   // a group's slice, zero past C
        for (int c = 0; c < NC; c++) out[c] = c0 + c < C ? row[c0 + c] : 0.f;
    };

    // per (list slot): the geometric sums (over groups, fp32 per (slot, quadrant, group) then double) and the channel sums
    std::vector<double> geo((size_t)R * 6, 0.0), fsum((size_t)R * C, 0.0);
    long checked = 0;
    for (int tile = 0; tile < ntiles; tile++) {
        const uint32_t r0 = ranges[2 * tile], len = ranges[2 * tile + 1] - r0;
        const int tx = tile % gx, ty = tile / gx;
        std::vector<double> want_f((size_t)len * C, 0.0), abs_f((size_t)len * C, 0.0);
        std::vector<int> depth_of(len, 0);
        for (int quad = 0; quad < 4; quad++)
            for (int grp = 0; grp < groups; grp++) {
                const int c0 = grp * NC;
                std::vector<FeatSums<NC>> sums(len);
                for (auto& s : sums) feat_sums_clear<NC>(s);
                for (int lane = 0; lane < 64; lane++) {
                    const int px = tx * kTile + (quad & 1) * 8 + (lane & 7), py = ty * kTile + (quad >> 1) * 8 + (lane >> 3);
                    if (px >= W || py >= H) continue;
                    const size_t pixel = (size_t)py * W + px;
                    const uint32_t n = ncon[pixel] < len ? ncon[pixel] : len;
                    const float pxf = (float)px, pyf = (float)py;
                    // ---- forward: the feature run, the colour run, the restatement
                    FeatPix<NC> p;
                    feat_pix_init<NC>(p, true);
                    FwdPix col;
                    fwd_pix_init(col, true);
                    double T = 1.0, D[NC], A[NC];
                    for (int c = 0; c < NC; c++) D[c] = A[c] = 0.0;
                    int k = 0;
                    for (uint32_t e = 0; e < n; e++) {
                        const uint32_t id = list[r0 + e];
                        const QSplat s = splat_of(id);
                        float fs[NC], Tb;
                        slice(&feat[(size_t)id * C], c0, fs);
                        const int code = feat_step<NC>(s, pxf, pyf, e + 1, n, fs, p);
                        if (fwd_step(s, pxf, pyf, e + 1, col, &Tb) != code) return fail("step code", (long)pixel, e, code, -1);
                        if (code == 1) {
                            bool inb;
                            const double alpha = (double)fwd_alpha(s, pxf, pyf, &inb);
                            for (int c = 0; c < NC; c++) {
                                D[c] += (double)fs[c] * alpha * T;
                                A[c] += std::fabs((double)fs[c]) * alpha * T;
                            }
                            T *= 1.0 - alpha;
                            k++;
                        }
                    }
                    if (bits(p.f.Tf) != bits(col.Tf) || bits(p.f.T) != bits(col.T)) return fail("T", (long)pixel, grp, p.f.Tf, col.Tf);
                    if (p.f.last != col.last) return fail("last", (long)pixel, grp, p.f.last, col.last);
                    if (std::fabs((double)p.f.Tf - T) > gamma_of(k) * T) return fail("T outside gamma(k)", (long)pixel, grp, p.f.Tf, T);
                    for (int c = 0; c < NC; c++)
                        if (std::fabs((double)p.acc[c] - D[c]) > gamma_of(2 * k + 2) * A[c])
                            return fail("channel sum outside gamma(2k+2)", (long)pixel, c0 + c, p.acc[c], D[c]);
                    checked++;
                    // ---- backward: back to front from the forward's own last contributor and final T
                    float gp[NC];
                    for (int c = 0; c < NC; c++) gp[c] = c0 + c < C ? g[(size_t)(c0 + c) * N + pixel] : 0.f;
                    FeatBwdPix<NC> b;
                    feat_bwd_pix_init<NC>(b, true, finalT[pixel], ncon[pixel], gp);
                    double Td = (double)finalT[pixel];
                    int steps = 0;
                    for (uint32_t e = n; e-- > 0;) {
                        const uint32_t id = list[r0 + e];
                        const QSplat s = splat_of(id);
                        float fs[NC];
                        slice(&feat[(size_t)id * C], c0, fs);
                        BwdEval ev;
                        const bool valid = bwd_test(s, pxf, pyf, e, b.b, ev);
                        if (feat_bwd_step<NC, true>(s, pxf, pyf, e, fs, b, sums[e]) != valid) return fail("bwd decision", (long)pixel, e, 0, 0);
                        if (!valid) continue;
                        steps++;
                        Td /= 1.0 - (double)ev.alpha;
                        if (depth_of[e] < steps) depth_of[e] = steps;
                        if (grp * NC < C)
                            for (int c = 0; c < NC && c0 + c < C; c++) {
                                const double term = (double)ev.alpha * Td * (double)gp[c];
                                want_f[(size_t)e * C + c0 + c] += term;
                                abs_f[(size_t)e * C + c0 + c] += std::fabs(term);
                            }
                    }
                }
                for (uint32_t e = 0; e < len; e++) {
                    const SplatSums& s = sums[e].s;
                    const float row[6] = {s.sx, s.sy, s.sxx, s.sxy, s.syy, s.sm};
                    for (int q = 0; q < 6; q++) geo[(size_t)(r0 + e) * 6 + q] += (double)row[q];
                    for (int c = 0; c < NC && c0 + c < C; c++) fsum[(size_t)(r0 + e) * C + c0 + c] += (double)sums[e].f[c];
                }
            }
        for (uint32_t e = 0; e < len; e++)
            for (int c = 0; c < C; c++) {
                const double got = fsum[(size_t)(r0 + e) * C + c], want = want_f[(size_t)e * C + c];
                if (std::fabs(got - want) > gamma_of(3 * depth_of[e] + 2 + 64) * abs_f[(size_t)e * C + c])
                    return fail("feature gradient sum outside its bound", r0 + e, c, got, want);
            }
    }
    // per Gaussian: slots ascending, in double
    std::vector<double> G6((size_t)P * 6, 0.0), GF((size_t)P * C, 0.0);
    for (int tile = 0; tile < ntiles; tile++)
        for (uint32_t e = ranges[2 * tile]; e < ranges[2 * tile + 1]; e++) {
            for (int q = 0; q < 6; q++) G6[(size_t)list[e] * 6 + q] += geo[(size_t)e * 6 + q];
            for (int c = 0; c < C; c++) GF[(size_t)list[e] * C + c] += fsum[(size_t)e * C + c];
        }
    for (int i = 0; i < P; i++) {
        SplatSums u;
        aux_sums_clear(u);
        const double* s = &G6[(size_t)i * 6];
        u.sx = (float)s[0];
        u.sy = (float)s[1];
        u.sxx = (float)s[2];
        u.sxy = (float)s[3];
        u.syy = (float)s[4];
        u.sm = (float)s[5];
        const SplatGrad d = splat_grad_of(splat_of((uint32_t)i), u);
        std::printf("%d %.9g %.9g %.9g %.9g %.9g %.9g", i, d.mx, d.my, d.cA, d.cB, d.cC, d.op);
        for (int c = 0; c < C; c++) std::printf(" %.9g", (float)GF[(size_t)i * C + c]);
        std::printf("\n");
    }
    std::printf("hostcheck_features: OK %d Gaussians, %d channels, %ld (pixel, group) runs\n", P, C, checked);
    return 0;
}
