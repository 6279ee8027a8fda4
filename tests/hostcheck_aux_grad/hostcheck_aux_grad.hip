// Host check of the gradients through the auxiliary maps (reduced-3dgs_amd/csrc/aux_math.h): a stand-alone program that runs
// the shared per-(pixel, entry) step (aux_bwd_step) and the per-Gaussian chain (aux_bwd_chain) on the CPU over the scene in
// the text file named on its command line, in the order the device pass sums -- per (list slot, 8x8 quadrant) in fp32, then
// per Gaussian over its slots ascending and quadrants 0..3 in double -- and prints one line per Gaussian:
//   id  dmean2D.x dmean2D.y  dmean3D.xyz  dopacity  dscale.xyz  drot.wxyz  z-sum
// tests/test_aux_grad_cpu.py writes the scene (a seeded one, from the oracle's state), compares the lines with
// tests/aux_grad_ref.py, and builds this file once plainly and once with -fsanitize=address,undefined on the host side.
//
// Input, whitespace separated:  W H P R ntiles f64 tan_fovx tan_fovy scale_modifier, view[16], proj[16],
//   ranges[ntiles][2], point_list[R], then per pixel (H*W): n_contrib final_T g_depth g_alpha g_median,
//   then per Gaussian (P): radius  x y conicA conicB conicC opacity z  mean3D[3] scale[3] rot[4].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reduced-3dgs_amd/csrc/aux_math.h"

using namespace r3;

namespace {

bool read_floats(FILE* f, float* p, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (std::fscanf(f, "%f", p + k) != 1) return false;
    return true;
}

struct Pixel {
    uint32_t n;
    float T, gD, gA, gM;
};

struct Gauss {
    int radius;
    float rec[7];   // x, y, conic A, B, C, opacity, z
    float mean[3], scale[3], rot[4];
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: hostcheck_aux_grad scene.txt\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int W, H, P, R, ntiles, f64;
    Camera cam{};
    if (std::fscanf(f, "%d %d %d %d %d %d %f %f %f", &W, &H, &P, &R, &ntiles, &f64, &cam.tan_fovx, &cam.tan_fovy,
                    &cam.scale_modifier) != 9 ||
        W < 1 || H < 1 || P < 0 || R < 0 || ntiles != ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile))
        return 2;
    if (!read_floats(f, cam.view, 16) || !read_floats(f, cam.proj, 16)) return 2;
    cam.W = W;
    cam.H = H;
    cam.gx = (W + kTile - 1) / kTile;
    cam.gy = (H + kTile - 1) / kTile;
    cam.focal_x = W / (2.0f * cam.tan_fovx);
    cam.focal_y = H / (2.0f * cam.tan_fovy);
    std::vector<uint32_t> ranges((size_t)ntiles * 2), list((size_t)R);
    for (uint32_t& v : ranges)
        if (std::fscanf(f, "%u", &v) != 1) return 2;
    for (uint32_t& v : list)
        if (std::fscanf(f, "%u", &v) != 1) return 2;
    std::vector<Pixel> pix((size_t)W * H);
    for (Pixel& p : pix)
        if (std::fscanf(f, "%u %f %f %f %f", &p.n, &p.T, &p.gD, &p.gA, &p.gM) != 5) return 2;
    std::vector<Gauss> gs((size_t)P);
    for (Gauss& g : gs) {
        if (std::fscanf(f, "%d", &g.radius) != 1 || !read_floats(f, g.rec, 7) || !read_floats(f, g.mean, 3) ||
            !read_floats(f, g.scale, 3) || !read_floats(f, g.rot, 4))
            return 2;
    }
    std::fclose(f);

    // the pixel pass: one row of seven fp32 sums per (list slot, quadrant), each pixel walked back to front
    std::vector<float> slab((size_t)R * kAuxQuads * kAuxRowFloats, 0.f);
    for (int tile = 0; tile < ntiles; tile++) {
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        if (r1 < r0 || r1 > (uint32_t)R) return 2;
        const int tx = tile % cam.gx, ty = tile / cam.gx;
        for (int quad = 0; quad < kAuxQuads; quad++) {
            std::vector<SplatSums> sums(r1 - r0);
            for (SplatSums& s : sums) aux_sums_clear(s);
            for (int lane = 0; lane < 64; lane++) {   // lanes in order: the wave's tree sum adds the same 64 terms
                const int px = tx * kTile + (quad & 1) * 8 + (lane & 7), py = ty * kTile + (quad >> 1) * 8 + (lane >> 3);
                if (px >= W || py >= H) continue;
                const Pixel& q = pix[(size_t)py * W + px];
                BwdPix p;
                aux_bwd_pix_init(p, true, q.T, q.n, q.gD, q.gA);
                for (uint32_t k = q.n < r1 - r0 ? q.n : r1 - r0; k-- > 0;) {
                    const uint32_t id = list[r0 + k];
                    if (id >= (uint32_t)P) return 2;
                    const float* r = gs[id].rec;
                    Splat s{r[0], r[1], r[2], r[3], r[4], r[5], 0.f, 0.f, 0.f};
                    const QSplat qs = scale_splat(s);
                    aux_bwd_step(aux_bwd_splat(qs.x, qs.y, qs.qa, qs.qb, qs.qc, qs.op, r[6]), (float)px, (float)py, k, p, q.gM, sums[k]);
                }
            }
            for (uint32_t k = 0; k < r1 - r0; k++) aux_row_of(sums[k], &slab[((size_t)(r0 + k) * kAuxQuads + quad) * kAuxRowFloats]);
        }
    }
    // the per-Gaussian sum (slots ascending, quadrants 0..3, double) and chain
    std::vector<std::vector<uint32_t>> slots((size_t)P);
    for (int tile = 0; tile < ntiles; tile++)
        for (uint32_t e = ranges[2 * tile]; e < ranges[2 * tile + 1]; e++) {
            if (list[e] >= (uint32_t)P) return 2;   // (entries behind every pixel's n_contrib were not looked at by the walk)
            slots[list[e]].push_back(e);
        }
    for (int i = 0; i < P; i++) {
        const Gauss& g = gs[(size_t)i];
        AuxGaussGrad o{};
        double sums[kAuxSums] = {0, 0, 0, 0, 0, 0, 0};
        if (g.radius > 0) {
            for (uint32_t e : slots[(size_t)i])   // ascending: tiles were visited in order
                for (int q = 0; q < kAuxQuads; q++)
                    for (int k = 0; k < kAuxSums; k++) sums[k] += (double)slab[((size_t)e * kAuxQuads + q) * kAuxRowFloats + k];
            if (f64)
                aux_bwd_chain<true>(cam, g.rec, sums, g.mean, g.scale, g.rot, nullptr, o);
            else
                aux_bwd_chain<false>(cam, g.rec, sums, g.mean, g.scale, g.rot, nullptr, o);
        }
        std::printf("%d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", i, o.mean2D[0], o.mean2D[1],
                    o.mean3D[0], o.mean3D[1], o.mean3D[2], o.opacity, o.scale[0], o.scale[1], o.scale[2], o.rot[0], o.rot[1],
                    o.rot[2], o.rot[3], g.radius > 0 ? (float)sums[6] : 0.f);
    }
    std::printf("hostcheck_aux_grad: OK %d Gaussians\n", P);
    return 0;
}
