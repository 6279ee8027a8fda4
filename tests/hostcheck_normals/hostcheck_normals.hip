// Host shim of the surface-normal unit: runs the __host__ __device__ arithmetic of reduced-3dgs_amd/csrc/normal_math.h on the
// CPU, element by element, the way reduced-3dgs_amd/csrc/normals.hip drives it (the backward in gather form: every pixel adds
// the shares its four neighbours hold for it).  Built by tests/hostcheck_build.py; with -DHOSTCHECK_NORMALS_MAIN a stand-alone
// program that sweeps every function over edge inputs (run plain and under ASan / UBSan by tests/test_normals_cpu.py).
#include "../../reduced-3dgs_amd/csrc/normal_math.h"

#include <cstdio>
#include <vector>

namespace {

double z_at(const float* depth, const float* alpha, size_t p) { return r3::normal_pixel_z(depth[p], alpha ? alpha[p] : 1.f, alpha != nullptr); }

bool interior(int x, int y, int W, int H) { return x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2; }

r3::DepthNormal centre(int x, int y, int W, int H, const r3::NormalRays& r, const float* depth, const float* alpha)
{
    const size_t p = (size_t)y * W + x;
    return r3::depth_normal_one(z_at(depth, alpha, p - W), z_at(depth, alpha, p + W), z_at(depth, alpha, p - 1), z_at(depth, alpha, p + 1),
                                r.x0 + x * r.dx, r.y0 + y * r.dy, r.dx, r.dy);
}

}  // namespace

extern "C" {

int hc_normal_axis(const float* s) { return r3::normal_axis(s); }
float hc_ndc2pix(float v, int S) { return r3::ndc2pix(v, S); }
void hc_ray(int W, int H, float tan_fovx, float tan_fovy, int x, int y, double* out)
{
    const r3::NormalRays r = r3::normal_rays(W, H, tan_fovx, tan_fovy);
    out[0] = r.x0 + x * r.dx;
    out[1] = r.y0 + y * r.dy;
}

void hc_gaussian_normals(int P, const float* means, const float* scales, const float* rot, int raw, const float* view,
                         const float* campos, float* out)
{
    for (int i = 0; i < P; i++) r3::gaussian_normal_one(view, campos, means + 3 * i, scales + 3 * i, rot + 4 * i, raw != 0, out + 3 * i);
}

void hc_gaussian_normals_bwd(int P, const float* means, const float* scales, const float* rot, int raw, const float* view,
                             const float* campos, const float* g, float* dq)
{
    for (int i = 0; i < P; i++)
        r3::gaussian_normal_bwd_one(view, campos, means + 3 * i, scales + 3 * i, rot + 4 * i, raw != 0, g + 3 * i, dq + 4 * i);
}

void hc_depth_normal(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha, const float* normal_map,
                     const float* weight, int scale_by_alpha, float* surf, double* loss)
{
    const r3::NormalRays r = r3::normal_rays(W, H, tan_fovx, tan_fovy);
    const size_t plane = (size_t)H * W;
    double sum = 0.0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            double n[3] = {0.0, 0.0, 0.0};
            if (interior(x, y, W, H)) {
                const r3::DepthNormal o = centre(x, y, W, H, r, depth, alpha);
                n[0] = o.n[0], n[1] = o.n[1], n[2] = o.n[2];
            }
            for (int k = 0; k < 3; k++) surf[k * plane + p] = (float)n[k];
            if (normal_map) {
                const float N[3] = {normal_map[p], normal_map[plane + p], normal_map[2 * plane + p]};
                sum += r3::normal_loss_term(weight ? (double)weight[p] : 1.0, scale_by_alpha && alpha ? (double)alpha[p] : 1.0, N, n);
            }
        }
    if (loss) *loss = sum / (double)plane;
}

void hc_depth_normal_bwd(int H, int W, float tan_fovx, float tan_fovy, const float* depth, const float* alpha,
                         const float* normal_map, const float* weight, int scale_by_alpha, float g_loss, const float* g_surf,
                         float* d_depth, float* d_alpha, float* d_normal)
{
    const r3::NormalRays r = r3::normal_rays(W, H, tan_fovx, tan_fovy);
    const size_t plane = (size_t)H * W;
    const double gl = normal_map ? (double)g_loss / (double)plane : 0.0;
    std::vector<double> to(4 * plane, 0.0);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            double n[3] = {0.0, 0.0, 0.0}, f = 0.0;
            if (interior(x, y, W, H)) {
                const r3::DepthNormal o = centre(x, y, W, H, r, depth, alpha);
                double g[3] = {0.0, 0.0, 0.0};
                if (g_surf) g[0] = g_surf[p], g[1] = g_surf[plane + p], g[2] = g_surf[2 * plane + p];
                if (gl != 0.0) {
                    f = -gl * (weight ? (double)weight[p] : 1.0) * (scale_by_alpha && alpha ? (double)alpha[p] : 1.0);
                    for (int k = 0; k < 3; k++) g[k] += f * normal_map[k * plane + p];
                }
                for (int k = 0; k < 3; k++) n[k] = o.n[k];
                r3::depth_normal_bwd_one(o, r.x0 + x * r.dx, r.y0 + y * r.dy, r.dx, r.dy, g, &to[4 * p]);
            }
            if (d_normal)
                for (int k = 0; k < 3; k++) d_normal[k * plane + p] = (float)(f * n[k]);
        }
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const double a = y >= 1 ? to[4 * (p - W) + 0] : 0.0, b = y + 1 < H ? to[4 * (p + W) + 1] : 0.0;
            const double c = x >= 1 ? to[4 * (p - 1) + 2] : 0.0, d = x + 1 < W ? to[4 * (p + 1) + 3] : 0.0;
            const double gz = ((a + b) + c) + d;
            double dd = gz, da = 0.0;
            if (alpha) {
                if (r3::normal_alpha_live(alpha[p])) {
                    dd = gz / (double)alpha[p];
                    da = -gz * (double)depth[p] / ((double)alpha[p] * (double)alpha[p]);
                } else {
                    dd = 0.0;
                }
            }
            if (d_depth) d_depth[p] = (float)dd;
            if (d_alpha) d_alpha[p] = (float)da;
        }
}

}  // extern "C"

#ifdef HOSTCHECK_NORMALS_MAIN
int main()
{
    double checksum = 0.0;
    int bad = 0;
    const float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.1f, -0.2f, 0.3f, 1}, campos[3] = {-0.1f, 0.2f, -0.3f};
    const float quats[6][4] = {{1, 0, 0, 0}, {0, 0, 0, 0}, {1e-20f, 0, 0, 0}, {1e15f, -1e15f, 3e14f, 1e10f}, {0.5f, 0.5f, 0.5f, 0.5f}, {0, 3, 0, 4}};
    const float scales[4][3] = {{1, 1, 1}, {2, 1, 1}, {3, 2, 1}, {0, 0, 0}};
    const float means[3][3] = {{0, 0, 5}, {-0.1f, 0.2f, -0.3f}, {1e6f, -1e6f, 1e6f}};
    for (auto& q : quats)
        for (auto& s : scales)
            for (auto& m : means)
                for (int raw = 0; raw < 2; raw++) {
                    float n[3], dq[4];
                    const float g[3] = {0.3f, -0.7f, 1.1f};
                    hc_gaussian_normals(1, m, s, q, raw, view, campos, n);
                    hc_gaussian_normals_bwd(1, m, s, q, raw, view, campos, g, dq);
                    for (float v : n) bad += !(v == v), checksum += v == v ? v : 0.0;
                    for (float v : dq) bad += !(v == v);
                }
    for (int H = 1; H <= 9; H += 2)
        for (int W = 1; W <= 11; W += 3) {
            const size_t plane = (size_t)H * W;
            std::vector<float> depth(plane), alpha(plane), N(3 * plane, 0.5f), w(plane, 1.f), gs(3 * plane, 1.f), surf(3 * plane),
                dd(plane), da(plane), dn(3 * plane);
            for (size_t p = 0; p < plane; p++) depth[p] = p % 5 ? 1.f + 0.1f * (float)(p % 7) : 0.f, alpha[p] = p % 3 ? 0.8f : (p % 2 ? 0.f : 5e-4f);
            for (int use_alpha = 0; use_alpha < 2; use_alpha++) {
                double loss = 0.0;
                const float* al = use_alpha ? alpha.data() : nullptr;
                hc_depth_normal(H, W, 0.6f, 0.4f, depth.data(), al, N.data(), w.data(), 1, surf.data(), &loss);
                hc_depth_normal_bwd(H, W, 0.6f, 0.4f, depth.data(), al, N.data(), w.data(), 1, 1.f, gs.data(), dd.data(),
                                    use_alpha ? da.data() : nullptr, dn.data());
                bad += !(loss == loss);
                checksum += loss;
                for (float v : surf) bad += !(v == v);
                for (float v : dd) bad += !(v == v);
                for (float v : dn) bad += !(v == v);
                if (use_alpha)
                    for (float v : da) bad += !(v == v);
            }
        }
    printf("checksum %.17g bad %d\n", checksum, bad);
    return bad != 0;
}
#endif
