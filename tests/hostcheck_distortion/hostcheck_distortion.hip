// Host check of the depth-distortion map and of the gradients through it (reduced-3dgs_amd/csrc/distortion_math.h): a
// stand-alone program that runs the shared steps on the CPU over the scene in the text file named on its command line.
//   forward : dist_step per (pixel, entry) front to back, depths relative to the tile's first list entry as the kernel has them;
//             one line per pixel:  pix  distortion  S1  S2     (the shifted moments the backward then reads)
//   backward: dist_bwd_step back to front in the order the device pass sums -- per (list slot, 8x8 quadrant) in fp32, then per
//             Gaussian over its slots ascending and quadrants 0..3 in double -- and aux_bwd_chain; one line per Gaussian:
//             id  dmean2D.x dmean2D.y  dmean3D.xyz  dopacity  dscale.xyz  drot.wxyz  z-sum
// tests/test_distortion_cpu.py writes the scene (a seeded one, from the oracle's state), compares the lines with
// tests/distortion_ref.py, and builds this file once plainly and once with -fsanitize=address,undefined on the host side.
//
// Input, whitespace separated:  W H P R ntiles f64 tan_fovx tan_fovy scale_modifier near far, view[16], proj[16],
//   ranges[ntiles][2], point_list[R], then per pixel (H*W): n_contrib final_T g,
//   then per Gaussian (P): radius  x y conicA conicB conicC opacity z  mean3D[3] scale[3] rot[4].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reduced-3dgs_amd/csrc/distortion_math.h"

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
    float T, g;
    float dist, S1, S2;   // the forward's results
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
        std::fprintf(stderr, "usage: hostcheck_distortion scene.txt\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int W, H, P, R, ntiles, f64;
    float near, far;
    Camera cam{};
    if (std::fscanf(f, "%d %d %d %d %d %d %f %f %f %f %f", &W, &H, &P, &R, &ntiles, &f64, &cam.tan_fovx, &cam.tan_fovy,
                    &cam.scale_modifier, &near, &far) != 11 ||
        W < 1 || H < 1 || P < 0 || R < 0 || ntiles != ((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile) ||
        !depth_map_valid(near, far))
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
    for (Pixel& p : pix) {
        if (std::fscanf(f, "%u %f %f", &p.n, &p.T, &p.g) != 3) return 2;
        p.dist = p.S1 = p.S2 = 0.f;
    }
    std::vector<Gauss> gs((size_t)P);
    for (Gauss& g : gs) {
        if (std::fscanf(f, "%d", &g.radius) != 1 || !read_floats(f, g.rec, 7) || !read_floats(f, g.mean, 3) ||
            !read_floats(f, g.scale, 3) || !read_floats(f, g.rot, 4))
            return 2;
    }
    std::fclose(f);
    for (int tile = 0; tile < ntiles; tile++) {
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        if (r1 < r0 || r1 > (uint32_t)R) return 2;
        for (uint32_t e = r0; e < r1; e++)
            if (list[e] >= (uint32_t)P) return 2;
    }
    // the mapping of a tile: relative to the view depth of its first list entry (1 for an empty list), as the kernels have it
    auto map_of = [&](int tile) {
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        return depth_map_of(near, far, r1 > r0 ? gs[list[r0]].rec[6] : 1.0f);
    };

    // the forward: every pixel front to back
    for (int py = 0; py < H; py++)
        for (int px = 0; px < W; px++) {
            const int tile = (py / kTile) * cam.gx + px / kTile;
            const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
            const DepthMap dm = map_of(tile);
            Pixel& q = pix[(size_t)py * W + px];
            DistPix p;
            dist_pix_init(p, true);
            for (uint32_t k = 0; k < r1 - r0 && k < q.n; k++) {
                const float* r = gs[list[r0 + k]].rec;
                const Splat s{r[0], r[1], r[2], r[3], r[4], r[5], 0.f, 0.f, 0.f};
                dist_step(s, r[6], dm, (float)px, (float)py, k + 1u, q.n, p);
            }
            q.dist = dist_value(p);
            q.S1 = dist_moment1(p);
            q.S2 = dist_moment2(p);
            std::printf("pix %d %.9g %.9g %.9g\n", py * W + px, q.dist, q.S1, q.S2);
        }

    // the backward's pixel pass: one row of seven fp32 sums per (list slot, quadrant), each pixel walked back to front
    std::vector<float> slab((size_t)R * kAuxQuads * kAuxRowFloats, 0.f);
    for (int tile = 0; tile < ntiles; tile++) {
        const uint32_t r0 = ranges[2 * tile], r1 = ranges[2 * tile + 1];
        const int tx = tile % cam.gx, ty = tile / cam.gx;
        const DepthMap dm = map_of(tile);
        for (int quad = 0; quad < kAuxQuads; quad++) {
            std::vector<SplatSums> sums(r1 - r0);
            for (SplatSums& s : sums) aux_sums_clear(s);
            for (int lane = 0; lane < 64; lane++) {
                const int px = tx * kTile + (quad & 1) * 8 + (lane & 7), py = ty * kTile + (quad >> 1) * 8 + (lane >> 3);
                if (px >= W || py >= H) continue;
                const Pixel& q = pix[(size_t)py * W + px];
                BwdPix p;
                dist_bwd_pix_init(p, true, q.T, q.n, q.g);
                const DistTotals tot{1.0f - q.T, q.S1, q.S2};
                for (uint32_t k = q.n < r1 - r0 ? q.n : r1 - r0; k-- > 0;) {
                    const float* r = gs[list[r0 + k]].rec;
                    const Splat s{r[0], r[1], r[2], r[3], r[4], r[5], 0.f, 0.f, 0.f};
                    const QSplat qs = scale_splat(s);
                    dist_bwd_step(aux_splat(qs.x, qs.y, qs.qa, qs.qb, qs.qc, qs.op, mapped_depth_shifted(dm, r[6])),
                                  mapped_depth_dz(dm, r[6]), (float)px, (float)py, k, p, tot, sums[k]);
                }
            }
            for (uint32_t k = 0; k < r1 - r0; k++) aux_row_of(sums[k], &slab[((size_t)(r0 + k) * kAuxQuads + quad) * kAuxRowFloats]);
        }
    }
    // the per-Gaussian sum (slots ascending, quadrants 0..3, double) and chain
    std::vector<std::vector<uint32_t>> slots((size_t)P);
    for (int tile = 0; tile < ntiles; tile++)
        for (uint32_t e = ranges[2 * tile]; e < ranges[2 * tile + 1]; e++) slots[list[e]].push_back(e);
    for (int i = 0; i < P; i++) {
        const Gauss& g = gs[(size_t)i];
        AuxGaussGrad o{};
        double sums[kAuxSums] = {0, 0, 0, 0, 0, 0, 0};
        if (g.radius > 0) {
            for (uint32_t e : slots[(size_t)i])
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
    std::printf("hostcheck_distortion: OK %d Gaussians\n", P);
    return 0;
}
