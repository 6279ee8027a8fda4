// camera_bwd.hip -- gradients of the image with respect to the camera: viewmatrix, projmatrix, campos
// (include/r3dgs_camera.h r3dgs_camera_backward; the arithmetic is camera_math.h), gfx950.  A pass of its own behind a
// backward: it reads the model, the forward's geometry blob and the per-Gaussian screen-space sums the backward wrote, and
// writes only the caller's three outputs and workspace.  No existing kernel takes part.
//
// A streaming reduction over the Gaussians into 27 numbers (12 of dL/dV, 12 of dL/dF, 3 of dL/dcampos; the other 8 of the
// 35 outputs are structural zeros), ~120 B per visible Gaussian and 4 B per culled one.  Two launches, no host wait, no
// allocation, no atomics:
//   1. camera_grad_kernel -- kCamBlock lanes per workgroup, one lane per Gaussian per trip of a grid-stride loop.  A lane
//      loads radii first and everything else only where radii > 0, issues all of a visible Gaussian's loads before the first
//      use, and keeps its 27 sums in double across its trips.  At the end: a wave reduction by shuffles in a fixed order,
//      one LDS step over the workgroup's waves in wave order, and one row of 27 doubles per workgroup into the workspace.
//   2. camera_finish_kernel -- one workgroup: lane k adds sum k of the rows in index order and the three outputs are written
//      whole, the structurally empty columns with zeros.
// The grid is a function of P alone (cam_rows), and with it the order of every addition: the same inputs give the same bits.
//
// r3dgs_camera_backward_maps -- the same pass for a loss on the replay maps (depth / alpha / median depth, distortion, feature
// maps) -- is camera_maps_kernel below: no colour, so no SH row, no blob and no campos; 24 sums (the view depth's own gradient
// joins column 2 of dL/dV); the same reduction, the same grid, and camera_finish_kernel over rows whose last three sums are 0.
#include <string>
#include <type_traits>

#include "../../include/r3dgs_camera.h"
#include "camera_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kCamBlock = 256;
constexpr int kCamWaves = kCamBlock / 64;
constexpr int kCamMaxRows = 512;   // workgroups at most (two per CU): beyond P = 131072 the lanes take several trips

inline int cam_rows(int P)
{
    const long long want = ((long long)P + kCamBlock - 1) / kCamBlock;
    return (int)(want < 1 ? 1 : want > kCamMaxRows ? kCamMaxRows : want);
}

struct CamGradArgs {
    int P, M, W, H;
    const int* degrees;
    const float* means3D;
    const float* shs;        // [P,M,3], or raw: features_dc [P,1,3]; nullptr: no SH colour
    const float* shs_rest;   // raw: features_rest [P,M-1,3]
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* view;
    const float* proj;
    const float* campos;
    float tan_fovx, tan_fovy, scale_modifier;
    const int* radii;
    const GRec* rec;
    const uint32_t* tiles;
    const GeomHeader* header;
    const float* sh_ddir;
    const float* dL_dmean2D;
    const float* dL_dconic;
    const float* dL_dcolor;
    double* rows;            // [gridDim.x][kCamSums]
};

// One Gaussian's SH row in global memory: [M][3] in one piece, or split as the model stores it (dc, then rest).
struct ShRowGlobal {
    const R3_GLOBAL float* first;   // coefficient 0
    const R3_GLOBAL float* rest;    // coefficients 1 .. M-1
    R3_HD float at(int e) const { return e < 3 ? first[e] : rest[e - 3]; }
};

template <bool F64, bool RAW>
__global__ __launch_bounds__(kCamBlock) void camera_grad_kernel(const CamGradArgs a)
{
    __shared__ double s_part[kCamWaves][kCamSums];
    using T = typename std::conditional<F64, double, float>::type;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t P = (size_t)a.P, M = (size_t)a.M;
    ViewParams vp;
    vp.tan_fovx = a.tan_fovx;
    vp.tan_fovy = a.tan_fovy;
    vp.W = a.W;
    vp.H = a.H;
    vp.scale_modifier = a.scale_modifier;
    const Camera cam = load_camera_from(global_ptr(a.view), global_ptr(a.proj), global_ptr(a.campos), vp);   // scalar loads
    const bool has_sh = a.shs != nullptr;
    const bool cached = has_sh && a.sh_ddir != nullptr && global_ptr(a.header)->sh_cache != 0u;   // wave-uniform
    const bool precomp = a.cov3D_precomp != nullptr;
    const int max_deg = M >= 16 ? 3 : M >= 9 ? 2 : M >= 4 ? 1 : 0;   // the degree M coefficients support

    double acc[kCamSums];
#pragma unroll
    for (int k = 0; k < kCamSums; k++) acc[k] = 0.0;

    for (size_t i = (size_t)blockIdx.x * kCamBlock + tid; i < P; i += (size_t)gridDim.x * kCamBlock) {
        if (global_ptr(a.radii)[i] <= 0) continue;   // culled: none of its other loads
        // every load of the Gaussian before the first use of any of them
        const uint32_t clamp_bits = global_ptr(a.rec)[i].width_clamp >> 16;
        const uint32_t ntile = global_ptr(a.tiles)[i];
        float m3[3], sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c6[6], g2[2], gcon[3], dcol[3], d9[9];
        for (int k = 0; k < 3; k++) m3[k] = global_ptr(a.means3D)[3 * i + k];
        if (precomp) {
            for (int k = 0; k < 6; k++) c6[k] = global_ptr(a.cov3D_precomp)[6 * i + k];
        } else {
            for (int k = 0; k < 3; k++) sc[k] = global_ptr(a.scales)[3 * i + k];
            for (int k = 0; k < 4; k++) q[k] = global_ptr(a.rotations)[4 * i + k];
        }
        g2[0] = global_ptr(a.dL_dmean2D)[3 * i];
        g2[1] = global_ptr(a.dL_dmean2D)[3 * i + 1];
        gcon[0] = global_ptr(a.dL_dconic)[4 * i];
        gcon[1] = global_ptr(a.dL_dconic)[4 * i + 1];
        gcon[2] = global_ptr(a.dL_dconic)[4 * i + 3];
        int deg = 0;
        dcol[0] = dcol[1] = dcol[2] = 0.f;
        if (has_sh) {
            deg = min(global_ptr(a.degrees)[i], max_deg);   // never past the coefficients the rows hold
            for (int k = 0; k < 3; k++) dcol[k] = global_ptr(a.dL_dcolor)[3 * i + k];
            if (cached) {
#pragma unroll
                for (int k = 0; k < 9; k++) d9[k] = global_ptr(a.sh_ddir)[9 * i + k];
            }
        }
        // a Gaussian binned into no tile got no colour: the forward left it neither clamp bits nor derivatives, and its
        // dL_dcolor is zero
        const int colour = (!has_sh || ntile == 0u) ? 0 : cached ? 1 : 2;
        ShRowGlobal row{nullptr, nullptr};
        if (has_sh) {   // (no arithmetic on a null pointer; a row of one coefficient has no rest and, at degree 0, reads none)
            row.first = global_ptr(a.shs) + (RAW ? 3 * i : 3 * M * i);
            row.rest = !RAW ? row.first + 3 : M > 1 ? global_ptr(a.shs_rest) + 3 * (M - 1) * i : nullptr;
        }
        camera_grad_gaussian<T>(cam, m3, sc, q, precomp ? c6 : nullptr, RAW, g2, gcon, dcol, clamp_bits, deg, colour, d9, row, acc);
    }

    // wave sums: lane L adds lane L + 32, 16, 8, 4, 2, 1 in this order
#pragma unroll
    for (int k = 0; k < kCamSums; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (tid < kCamSums) {
        double v = s_part[0][tid];
#pragma unroll
        for (int w = 1; w < kCamWaves; w++) v += s_part[w][tid];
        global_ptr(a.rows)[(size_t)blockIdx.x * kCamSums + tid] = v;
    }
}

__global__ __launch_bounds__(64) void camera_finish_kernel(const double* __restrict__ rows, int nrows, float* dL_dview,
                                                           float* dL_dproj, float* dL_dcampos)
{
    __shared__ double s_sum[kCamSums];
    const int tid = threadIdx.x;
    if (tid < kCamSums) {
        double v = 0.0;
        for (int r = 0; r < nrows; r++) v += global_ptr(rows)[(size_t)r * kCamSums + tid];
        s_sum[tid] = v;
    }
    __syncthreads();
    if (tid < 16) {
        if (dL_dview) dL_dview[tid] = camera_view_entry(s_sum, tid);
        if (dL_dproj) dL_dproj[tid] = camera_proj_entry(s_sum, tid);
    }
    if (tid < 3 && dL_dcampos) dL_dcampos[tid] = (float)s_sum[24 + tid];
}

// ---- the camera pass of the replay maps (r3dgs_camera_backward_maps; camera_math.h camera_maps_gaussian) ----------------
// camera_grad_kernel without a colour: no SH row, no blob, no campos; three per-Gaussian gradient inputs, any of them nullptr
// (zero).  24 double sums per lane, the same wave / workgroup reduction in the same order, and rows of kCamSums doubles -- the
// last three zero -- so that camera_finish_kernel finishes both passes.
struct CamMapsArgs {
    int P, W, H;
    const float* means3D;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* view;
    const float* proj;
    float tan_fovx, tan_fovy, scale_modifier;
    const int* radii;
    const float* dL_dmean2D;   // [P,3] or nullptr
    const float* dL_dconic;    // [P,4] or nullptr
    const float* dL_dz;        // [P] or nullptr
    double* rows;              // [gridDim.x][kCamSums]
};

template <bool F64>
__global__ __launch_bounds__(kCamBlock) void camera_maps_kernel(const CamMapsArgs a)
{
    __shared__ double s_part[kCamWaves][kCamMapSums];
    using T = typename std::conditional<F64, double, float>::type;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t P = (size_t)a.P;
    ViewParams vp;
    vp.tan_fovx = a.tan_fovx;
    vp.tan_fovy = a.tan_fovy;
    vp.W = a.W;
    vp.H = a.H;
    vp.scale_modifier = a.scale_modifier;
    // scalar loads (campos: the view matrix's first three words stand in -- nothing of this pass looks at it)
    const Camera cam = load_camera_from(global_ptr(a.view), global_ptr(a.proj), global_ptr(a.view), vp);
    const bool precomp = a.cov3D_precomp != nullptr;
    const bool has_g2 = a.dL_dmean2D != nullptr, has_con = a.dL_dconic != nullptr, has_z = a.dL_dz != nullptr;   // wave-uniform

    double acc[kCamMapSums];
#pragma unroll
    for (int k = 0; k < kCamMapSums; k++) acc[k] = 0.0;

    for (size_t i = (size_t)blockIdx.x * kCamBlock + tid; i < P; i += (size_t)gridDim.x * kCamBlock) {
        if (global_ptr(a.radii)[i] <= 0) continue;   // culled: none of its other loads
        // every load of the Gaussian before the first use of any of them
        float m3[3], sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c6[6], g2[2] = {0.f, 0.f}, gcon[3] = {0.f, 0.f, 0.f};
        float gz = 0.f;
        for (int k = 0; k < 3; k++) m3[k] = global_ptr(a.means3D)[3 * i + k];
        if (precomp) {
            for (int k = 0; k < 6; k++) c6[k] = global_ptr(a.cov3D_precomp)[6 * i + k];
        } else {
            for (int k = 0; k < 3; k++) sc[k] = global_ptr(a.scales)[3 * i + k];
            for (int k = 0; k < 4; k++) q[k] = global_ptr(a.rotations)[4 * i + k];
        }
        if (has_g2) {
            g2[0] = global_ptr(a.dL_dmean2D)[3 * i];
            g2[1] = global_ptr(a.dL_dmean2D)[3 * i + 1];
        }
        if (has_con) {
            gcon[0] = global_ptr(a.dL_dconic)[4 * i];
            gcon[1] = global_ptr(a.dL_dconic)[4 * i + 1];
            gcon[2] = global_ptr(a.dL_dconic)[4 * i + 3];
        }
        if (has_z) gz = global_ptr(a.dL_dz)[i];
        camera_maps_gaussian<T>(cam, m3, sc, q, precomp ? c6 : nullptr, g2, gcon, gz, acc);
    }

    // wave sums: lane L adds lane L + 32, 16, 8, 4, 2, 1 in this order
#pragma unroll
    for (int k = 0; k < kCamMapSums; k++) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (tid < kCamSums) {
        double v = 0.0;   // (sums 24 .. 26 of a row: campos, which this pass does not have)
        if (tid < kCamMapSums) {
            v = s_part[0][tid];
#pragma unroll
            for (int w = 1; w < kCamWaves; w++) v += s_part[w][tid];
        }
        global_ptr(a.rows)[(size_t)blockIdx.x * kCamSums + tid] = v;
    }
}

}  // namespace

}  // namespace r3

extern "C" {

size_t r3dgs_camera_backward_maps_workspace_bytes(int P) { return r3dgs_camera_backward_workspace_bytes(P); }

int r3dgs_camera_backward_maps(int P, int width, int height, const float* means3D, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                               const float* projmatrix, float tan_fovx, float tan_fovy, const int* radii,
                               const float* dL_dmean2D, const float* dL_dconic, const float* dL_dz, float* dL_dviewmatrix,
                               float* dL_dprojmatrix, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (P < 0 || width < 1 || height < 1)
            throw Error("camera_backward_maps: need P >= 0 and width, height >= 1, got P = " + std::to_string(P) + ", " +
                        std::to_string(width) + "x" + std::to_string(height));
        if (!dL_dviewmatrix && !dL_dprojmatrix) return 0;
        if (P == 0 || (!dL_dmean2D && !dL_dconic && !dL_dz)) {   // zeros, nothing is read
            if (dL_dviewmatrix) R3_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), s));
            if (dL_dprojmatrix) R3_HIP(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), s));
            return 0;
        }
        if (!workspace) throw Error("camera_backward_maps: the workspace must not be NULL");
        if (!means3D || !radii || !viewmatrix || !projmatrix)
            throw Error("camera_backward_maps: means3D, radii, viewmatrix and projmatrix must not be NULL");
        if (!cov3D_precomp && (!scales || !rotations))
            throw Error("camera_backward_maps: need scales and rotations, or cov3D_precomp");
        Carver c(workspace);
        const int nrows = cam_rows(P);
        CamMapsArgs a;
        a.P = P;
        a.W = width;
        a.H = height;
        a.means3D = means3D;
        a.scales = scales;
        a.rotations = rotations;
        a.cov3D_precomp = cov3D_precomp;
        a.view = viewmatrix;
        a.proj = projmatrix;
        a.tan_fovx = tan_fovx;
        a.tan_fovy = tan_fovy;
        a.scale_modifier = scale_modifier;
        a.radii = radii;
        a.dL_dmean2D = dL_dmean2D;
        a.dL_dconic = dL_dconic;
        a.dL_dz = dL_dz;
        a.rows = c.take<double>((size_t)nrows * kCamSums);
        if (g_f64_chain.get() != 0)
            hipLaunchKernelGGL(camera_maps_kernel<true>, dim3(nrows), dim3(kCamBlock), 0, s, a);
        else
            hipLaunchKernelGGL(camera_maps_kernel<false>, dim3(nrows), dim3(kCamBlock), 0, s, a);
        check_launch("camera backward of the maps, per-Gaussian pass", s, false);
        hipLaunchKernelGGL(camera_finish_kernel, dim3(1), dim3(64), 0, s, a.rows, nrows, dL_dviewmatrix, dL_dprojmatrix,
                           (float*)nullptr);
        check_launch("camera backward of the maps, finish", s, false);
        return 0;
    });
}

size_t r3dgs_camera_backward_workspace_bytes(int P)
{
    if (P <= 0) return 0;
    return (size_t)r3::cam_rows(P) * r3::kCamSums * sizeof(double) + r3::kAlign;
}

int r3dgs_camera_backward(int P, const int* D, int M, int width, int height, const float* means3D, const float* shs,
                          const float* shs_rest, const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, int raw_params, const float* viewmatrix, const float* projmatrix,
                          const float* campos, float tan_fovx, float tan_fovy, const int* radii, char* geom_buffer,
                          const float* dL_dmean2D, const float* dL_dconic, const float* dL_dcolor, float* dL_dviewmatrix,
                          float* dL_dprojmatrix, float* dL_dcampos, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (P < 0 || width < 1 || height < 1)
            throw Error("camera_backward: need P >= 0 and width, height >= 1, got P = " + std::to_string(P) + ", " +
                        std::to_string(width) + "x" + std::to_string(height));
        if (!dL_dviewmatrix && !dL_dprojmatrix && !dL_dcampos) return 0;
        if (P == 0) {   // zeros, nothing is read
            if (dL_dviewmatrix) R3_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), s));
            if (dL_dprojmatrix) R3_HIP(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), s));
            if (dL_dcampos) R3_HIP(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), s));
            return 0;
        }
        if (!geom_buffer) throw Error("camera_backward: the geometry buffer must not be NULL");
        if (!workspace) throw Error("camera_backward: the workspace must not be NULL");
        if (!means3D || !radii || !viewmatrix || !projmatrix || !campos)
            throw Error("camera_backward: means3D, radii, viewmatrix, projmatrix and campos must not be NULL");
        if (!dL_dmean2D || !dL_dconic) throw Error("camera_backward: dL_dmean2D and dL_dconic must not be NULL");
        if (raw_params) {
            if (cov3D_precomp) throw Error("camera_backward: raw parameters and cov3D_precomp exclude each other");
            if (!scales || !rotations) throw Error("camera_backward: the raw-parameter form needs scales and rotations");
            if (!shs) throw Error("camera_backward: the raw-parameter form needs features_dc");
            if (M > 1 && !shs_rest) throw Error("camera_backward: features_rest must not be NULL for M > 1");
        } else if (!cov3D_precomp && (!scales || !rotations)) {
            throw Error("camera_backward: need scales and rotations, or cov3D_precomp");
        }
        if (shs && (M < 1 || M > 16)) throw Error("camera_backward: M must be 1 .. 16 with SH colours, got " + std::to_string(M));
        if (shs && (!D || !dL_dcolor)) throw Error("camera_backward: SH colours need the degrees and dL_dcolor");
        // the geometry blob as the forward carved it (the SH direction derivatives lie behind the depth sort's temp storage,
        // whose size the forward of this P has asked for and cached: no host work here)
        const GeomState geom = GeomState::carve(geom_buffer, (size_t)P, cached_depth_temp((size_t)P));
        Carver c(workspace);
        const int nrows = cam_rows(P);

        CamGradArgs a;
        a.P = P;
        a.M = shs ? M : 0;
        a.W = width;
        a.H = height;
        a.degrees = D;
        a.means3D = means3D;
        a.shs = shs;
        a.shs_rest = raw_params ? shs_rest : nullptr;
        a.scales = scales;
        a.rotations = rotations;
        a.cov3D_precomp = cov3D_precomp;
        a.view = viewmatrix;
        a.proj = projmatrix;
        a.campos = campos;
        a.tan_fovx = tan_fovx;
        a.tan_fovy = tan_fovy;
        a.scale_modifier = scale_modifier;
        a.radii = radii;
        a.rec = geom.rec;
        a.tiles = geom.tiles;
        a.header = geom.header;
        a.sh_ddir = geom.sh_ddir;
        a.dL_dmean2D = dL_dmean2D;
        a.dL_dconic = dL_dconic;
        a.dL_dcolor = dL_dcolor;
        a.rows = c.take<double>((size_t)nrows * kCamSums);
        const bool f64 = g_f64_chain.get() != 0;
        if (raw_params) {
            if (f64)
                hipLaunchKernelGGL((camera_grad_kernel<true, true>), dim3(nrows), dim3(kCamBlock), 0, s, a);
            else
                hipLaunchKernelGGL((camera_grad_kernel<false, true>), dim3(nrows), dim3(kCamBlock), 0, s, a);
        } else {
            if (f64)
                hipLaunchKernelGGL((camera_grad_kernel<true, false>), dim3(nrows), dim3(kCamBlock), 0, s, a);
            else
                hipLaunchKernelGGL((camera_grad_kernel<false, false>), dim3(nrows), dim3(kCamBlock), 0, s, a);
        }
        check_launch("camera backward, per-Gaussian pass", s, false);
        hipLaunchKernelGGL(camera_finish_kernel, dim3(1), dim3(64), 0, s, a.rows, nrows, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos);
        check_launch("camera backward, finish", s, false);
        return 0;
    });
}

}  // extern "C"
