// Host check of the maps' camera pass (reduced-3dgs_amd/csrc/camera_math.h camera_maps_gaussian): a shared library, built by
// tests/hostcheck_build.build_shim, that runs on the CPU the per-Gaussian function a lane of camera_maps_kernel runs, and --
// for the bit-for-bit comparison at dL_dz = 0 -- the colour route's camera_grad_gaussian with a zero colour gradient.
// Each visible Gaussian's share is formed in a zeroed row of its own, so that the caller sees the shares themselves:
//   sums[k]  += share[k]       (double, in index order)
//   abs[k]   += |share[k]|     (the scale a sum over many Gaussians in another order is held against)
#include <cmath>
#include <cstdint>

#include "../../reduced-3dgs_amd/csrc/camera_math.h"

using namespace r3;

namespace {

Camera camera_of(int W, int H, float tan_fovx, float tan_fovy, float scale_modifier, const float* view, const float* proj)
{
    Camera cam{};
    for (int k = 0; k < 16; k++) {
        cam.view[k] = view[k];
        cam.proj[k] = proj[k];
    }
    cam.tan_fovx = tan_fovx;
    cam.tan_fovy = tan_fovy;
    cam.W = W;
    cam.H = H;
    cam.gx = (W + kTile - 1) / kTile;
    cam.gy = (H + kTile - 1) / kTile;
    cam.focal_y = H / (2.0f * tan_fovy);
    cam.focal_x = W / (2.0f * tan_fovx);
    cam.scale_modifier = scale_modifier;
    return cam;
}

}  // namespace

extern "C" {

int hc_cam_map_sums() { return kCamMapSums; }

// colour_route != 0: camera_grad_gaussian with dL_dcolor = 0 and no SH colour (gz is ignored) instead of camera_maps_gaussian.
// shares (optional): [P][24], the rows themselves (zero rows for culled Gaussians).
void hc_camera_maps(int P, int f64, int colour_route, int W, int H, float tan_fovx, float tan_fovy, float scale_modifier,
                    const float* view, const float* proj, const int* radii, const float* means3D, const float* scales,
                    const float* rotations, const float* cov3D, const float* g2, const float* gcon, const float* gz, double* sums,
                    double* abs_sums, double* shares)
{
    const Camera cam = camera_of(W, H, tan_fovx, tan_fovy, scale_modifier, view, proj);
    for (int k = 0; k < kCamMapSums; k++) sums[k] = abs_sums[k] = 0.0;
    const float zero3[3] = {0.f, 0.f, 0.f}, zero9[9] = {0.f};
    for (int i = 0; i < P; i++) {
        double row[kCamSums];
        for (int k = 0; k < kCamSums; k++) row[k] = 0.0;
        if (radii[i] > 0) {
            const float* c6 = cov3D ? cov3D + 6 * (size_t)i : nullptr;
            const float* sc = scales ? scales + 3 * (size_t)i : zero3;
            const float* q = rotations ? rotations + 4 * (size_t)i : zero9;
            const float* m3 = means3D + 3 * (size_t)i;
            if (colour_route) {
                if (f64)
                    camera_grad_gaussian<double>(cam, m3, sc, q, c6, false, g2 + 2 * (size_t)i, gcon + 3 * (size_t)i, zero3, 0u, 0, 0,
                                                 zero9, ShRowPlain{zero9}, row);
                else
                    camera_grad_gaussian<float>(cam, m3, sc, q, c6, false, g2 + 2 * (size_t)i, gcon + 3 * (size_t)i, zero3, 0u, 0, 0,
                                                zero9, ShRowPlain{zero9}, row);
            } else if (f64) {
                camera_maps_gaussian<double>(cam, m3, sc, q, c6, g2 + 2 * (size_t)i, gcon + 3 * (size_t)i, gz[i], row);
            } else {
                camera_maps_gaussian<float>(cam, m3, sc, q, c6, g2 + 2 * (size_t)i, gcon + 3 * (size_t)i, gz[i], row);
            }
        }
        for (int k = 0; k < kCamMapSums; k++) {
            sums[k] += row[k];
            abs_sums[k] += std::fabs(row[k]);
            if (shares) shares[(size_t)i * kCamMapSums + k] = row[k];
        }
    }
}

// the sums -> the two outputs in the inputs' layout (camera_finish_kernel's own functions)
void hc_camera_maps_entries(const double* sums24, float* dL_dview, float* dL_dproj)
{
    double s[kCamSums];
    for (int k = 0; k < kCamSums; k++) s[k] = k < kCamMapSums ? sums24[k] : 0.0;
    for (int k = 0; k < 16; k++) {
        dL_dview[k] = camera_view_entry(s, k);
        dL_dproj[k] = camera_proj_entry(s, k);
    }
}

}  // extern "C"
