// Host check of the camera gradients (reduced-3dgs_amd/csrc/camera_math.h): a stand-alone program that runs the per-Gaussian
// function a lane of camera_grad_kernel runs (camera_grad_gaussian) on the CPU over the scene in the text file named on its
// command line, adds the 27 sums in double in index order and prints the 35 numbers of the three outputs, one per line:
//   dL_dviewmatrix[16], dL_dprojmatrix[16], dL_dcampos[3]
// tests/test_camera_grad_cpu.py writes the scenes (seeded, from the oracle's state), compares the lines with
// tests/camera_grad_ref.py, and builds this file once plainly and once with -fsanitize=address,undefined on the host side.
//
// Input, whitespace separated:  W H P M f64 mode tan_fovx tan_fovy scale_modifier, view[16], proj[16], campos[3], then per
// Gaussian (P):  radius clamp_bits degree colour  mean3D[3]  geometry  g2x g2y  gA gB gC  dcolor[3]  d9[9]  sh[3 M]
//   mode 0: geometry = scale[3] rot[4] activated;  1: cov3D[6];  2: scale[3] rot[4] RAW (activated here)
//   colour 0: none (precomputed colours / a Gaussian without a colour), 1: d9 holds the derivatives, 2: evaluate them from sh
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reduced-3dgs_amd/csrc/camera_math.h"

using namespace r3;

namespace {

bool read_floats(FILE* f, float* p, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (std::fscanf(f, "%f", p + k) != 1) return false;
    return true;
}

template <class T>
void run(const Camera& cam, int mode, int M, const std::vector<int>& head, const std::vector<float>& rows, size_t stride, double* acc)
{
    const size_t P = head.size() / 4;
    for (size_t i = 0; i < P; i++) {
        if (head[4 * i] <= 0) continue;   // culled
        const float* r = rows.data() + i * stride;
        const float* m3 = r;
        const float* geo = r + 3;
        const float* tail = geo + (mode == 1 ? 6 : 7);
        const ShRowPlain sh{tail + 17};
        camera_grad_gaussian<T>(cam, m3, geo, geo + 3, mode == 1 ? geo : nullptr, mode == 2, tail, tail + 2, tail + 5,
                                (uint32_t)head[4 * i + 1], head[4 * i + 2], M > 0 ? head[4 * i + 3] : 0, tail + 8, sh, acc);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: hostcheck_camera scene.txt\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int W, H, P, M, f64, mode;
    Camera cam{};
    if (std::fscanf(f, "%d %d %d %d %d %d %f %f %f", &W, &H, &P, &M, &f64, &mode, &cam.tan_fovx, &cam.tan_fovy,
                    &cam.scale_modifier) != 9 ||
        W < 1 || H < 1 || P < 0 || M < 0 || M > 16 || mode < 0 || mode > 2) {
        std::fclose(f);
        return 2;
    }
    if (!read_floats(f, cam.view, 16) || !read_floats(f, cam.proj, 16) || !read_floats(f, cam.campos, 3)) {
        std::fclose(f);
        return 2;
    }
    cam.W = W;
    cam.H = H;
    cam.gx = (W + kTile - 1) / kTile;
    cam.gy = (H + kTile - 1) / kTile;
    cam.focal_y = H / (2.0f * cam.tan_fovy);
    cam.focal_x = W / (2.0f * cam.tan_fovx);
    const size_t stride = 3 + (mode == 1 ? 6 : 7) + 2 + 3 + 3 + 9 + 3 * (size_t)M;
    std::vector<int> head(4 * (size_t)P);
    std::vector<float> rows((size_t)P * stride);
    for (int i = 0; i < P; i++) {
        for (int k = 0; k < 4; k++)
            if (std::fscanf(f, "%d", &head[4 * (size_t)i + k]) != 1) {
                std::fclose(f);
                return 2;
            }
        if (!read_floats(f, rows.data() + (size_t)i * stride, stride)) {
            std::fclose(f);
            return 2;
        }
    }
    std::fclose(f);
    double acc[kCamSums];
    for (int k = 0; k < kCamSums; k++) acc[k] = 0.0;
    if (f64)
        run<double>(cam, mode, M, head, rows, stride, acc);
    else
        run<float>(cam, mode, M, head, rows, stride, acc);
    for (int k = 0; k < 16; k++) std::printf("%.9g\n", camera_view_entry(acc, k));
    for (int k = 0; k < 16; k++) std::printf("%.9g\n", camera_proj_entry(acc, k));
    for (int k = 0; k < 3; k++) std::printf("%.9g\n", (float)acc[24 + k]);
    std::printf("hostcheck_camera: OK (%d Gaussians, mode %d, %s chain)\n", P, mode, f64 ? "double" : "fp32");
    return 0;
}
