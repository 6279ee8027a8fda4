// aux_bwd.hip -- gradients through the depth, alpha and median-depth maps (include/r3dgs_aux.h r3dgs_aux_maps_backward;
// the arithmetic is aux_math.h), gfx950.  A replay pass (DESIGN.md "Replay passes"): it reads the three state blobs and
// writes only the caller's outputs and workspace.
//
// Four launches on the caller's stream, no host wait, no allocation, no atomics:
//   1. aux_bwd_pixel_kernel -- the walk (replay_walk.h) back to front from ImageState::quad_depth, with T recovered from
//      final_T by division, as the backward blend recovers it.  The per-(pixel, entry) step is the backward blend's own
//      (bwd_test / bwd_accumulate through aux_math.h) on a splat of colour (z, 1, 0) and a pixel gradient (g_D, g_A, 0);
//      build.py compiles this unit with blend.hip's flags.  Per entry some lane blended, the wave reduces seven sums (2 for
//      the pixel mean, 3 for the conic, 1 for the opacity, 1 for z) into the entry's slab row (aux_bwd_stage.h).
//   2, 3. the (Gaussian id, list slot) keys and their stable sort by id (pair_sort.h; temp storage from the workspace).
//   4. aux_bwd_gauss_kernel -- one lane per Gaussian: its run of the sorted keys, its rows added in sorted order (list slot
//      ascending, quadrant 0..3) in double, then the per-Gaussian chain (aux_math.h aux_bwd_chain).  A Gaussian that lost
//      pairs to an overflowing reservation (its run is shorter than its tiles_touched) gets zero sums, as the colour
//      backward gives it zero 2D-stage gradients (preprocess_bwd.hip).
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
#include <string>

#include "../../include/r3dgs_aux.h"
#include "aux_bwd_stage.h"
#include "aux_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

struct AuxBwdArgs : WalkArgs {
    const float* g_depth;    // [H*W] or nullptr (zero)
    const float* g_alpha;
    const float* g_median;
    float* slab;             // [R][4][8]
};

__global__ __launch_bounds__(64) void aux_bwd_pixel_kernel(const AuxBwdArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    __shared__ float4 s_out[kWalkChunk][2];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const WalkSpan sp = load_walk_span(a, q);
    const uint32_t len = sp.len;
    R3_GLOBAL float4* const rows = reinterpret_cast<R3_GLOBAL float4*>(global_ptr(a.slab));
    slab_zero_behind(rows, sp, q.quad, lane);
    if (len == 0u) return;

    const float pxf = q.pxf, pyf = q.pyf;
    BwdPix p;
    float gM = 0.f;
    {
        float T = 1.f, gD = 0.f, gA = 0.f;
        uint32_t n = 0u;
        if (q.inside) {
            T = global_ptr(a.final_T)[q.pix];
            n = global_ptr(a.n_contrib)[q.pix];
            if (a.g_depth) gD = global_ptr(a.g_depth)[q.pix];
            if (a.g_alpha) gA = global_ptr(a.g_alpha)[q.pix];
            if (a.g_median) gM = global_ptr(a.g_median)[q.pix];
        }
        aux_bwd_pix_init(p, q.inside, T, n, gD, gA);
    }

    // software pipeline: the records of the next (shallower) chunk are gathered into registers while a chunk is walked
    uint32_t nxz = 0u;
    auto gather = [&](uint32_t k) {   // k: position in the list
        const WalkGather g = gather_rec(a.point_list + sp.first, a.rec, a.P, k, len);
        if (g.have) nxz = global_ptr(a.depth_key)[g.id];
        return g;
    };
    const uint32_t cfirst = ((len - 1u) / kWalkChunk) * kWalkChunk;
    WalkGather nx = gather(cfirst + (uint32_t)lane);
    SplatSums sg;
    aux_sums_clear(sg);
    for (uint32_t cbase = cfirst;; cbase -= kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, __uint_as_float(nxz), 0.f);
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        if (cbase >= kWalkChunk) nx = gather(cbase - kWalkChunk + (uint32_t)lane);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk some lane blended
        while (mask) {   // back to front: highest set bit first
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            QSplat s = load_splat_z(s_rec[j]);
            s.g = 1.f;   // colour (z, 1, 0): aux_math.h aux_bwd_splat
            BwdEval e;
            const bool valid = bwd_test(s, pxf, pyf, cbase + (uint32_t)j, p, e);
            if (valid) aux_bwd_apply(s, e, p, gM, sg);
            if (__ballot(valid) != 0ull) {
                slab_park_sums(s_out, j, lane, sg);
                contributed |= 1ull << j;
                aux_sums_clear(sg);
            }
        }
        __syncthreads();
        slab_store_chunk(rows, s_out, sp, q.quad, cbase, lane, contributed);
        if (cbase == 0u) break;
    }
}

struct AuxGaussArgs {
    const GRec* rec;
    const int* radii;
    const uint32_t* tiles;   // [P] tiles_touched: the pairs the forward wanted for the Gaussian
    const uint32_t* keys;    // [R] sorted ids
    const uint32_t* slots;   // [R] their list slots
    const float* slab;
    const float *view, *proj;
    const float *means3D, *scales, *rotations, *cov3D_precomp;
    float tan_fovx, tan_fovy, scale_modifier;
    int W, H;
    uint32_t P, R;
    float *dL_dmeans2D, *dL_dmeans3D, *dL_dopacity, *dL_dscales, *dL_drotations, *dL_dcov3D;
};

template <bool F64>
__global__ __launch_bounds__(64) void aux_bwd_gauss_kernel(const AuxGaussArgs a)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= a.P) return;
    AuxGaussGrad o;
    gauss_grad_clear(o);
    if (global_ptr(a.radii)[i] > 0) {
        const uint32_t lo = run_begin(a.keys, a.R, i);
        double sums[kAuxSums];
        for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        uint32_t j = lo;
        for (; j < a.R && global_ptr(a.keys)[j] == i; j++) {   // the run, counted as it is summed
            const uint32_t slot = global_ptr(a.slots)[j];
            if (slot >= a.R) continue;
            const auto* rows = reinterpret_cast<const R3_GLOBAL float4*>(global_ptr(a.slab)) + (size_t)slot * kAuxQuads * 2;
#pragma unroll
            for (int q = 0; q < kAuxQuads; q++) {
                const float4 r0 = rows[2 * q], r1 = rows[2 * q + 1];
                sums[0] += (double)r0.x;
                sums[1] += (double)r0.y;
                sums[2] += (double)r0.z;
                sums[3] += (double)r0.w;
                sums[4] += (double)r1.x;
                sums[5] += (double)r1.y;
                sums[6] += (double)r1.z;
            }
        }
        // A Gaussian whose pairs did not all fit the pass's pair reservation (the farthest pairs were dropped and the pass is
        // flagged) gets zero 2D-stage gradients instead of a partial sum, as in the colour backward (preprocess_bwd.hip).
        if (j - lo != global_ptr(a.tiles)[i])
            for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        Camera cam;
        for (int k = 0; k < 16; k++) {
            cam.view[k] = global_ptr(a.view)[k];
            cam.proj[k] = global_ptr(a.proj)[k];
        }
        cam.campos[0] = cam.campos[1] = cam.campos[2] = 0.f;   // (no term of this chain looks at it)
        cam.tan_fovx = a.tan_fovx;
        cam.tan_fovy = a.tan_fovy;
        cam.focal_y = a.H / (2.0f * a.tan_fovy);
        cam.focal_x = a.W / (2.0f * a.tan_fovx);
        cam.W = a.W;
        cam.H = a.H;
        cam.gx = (a.W + kTile - 1) / kTile;
        cam.gy = (a.H + kTile - 1) / kTile;
        cam.scale_modifier = a.scale_modifier;
        const GRec r = global_ptr(a.rec)[i];
        const float rec6[6] = {r.x, r.y, r.cA, r.cB, r.cC, r.op};
        float m3[3], sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c6[6];
        for (int k = 0; k < 3; k++) m3[k] = global_ptr(a.means3D)[3 * (size_t)i + k];
        if (a.cov3D_precomp) {
            for (int k = 0; k < 6; k++) c6[k] = global_ptr(a.cov3D_precomp)[6 * (size_t)i + k];
        } else {
            for (int k = 0; k < 3; k++) sc[k] = global_ptr(a.scales)[3 * (size_t)i + k];
            for (int k = 0; k < 4; k++) q[k] = global_ptr(a.rotations)[4 * (size_t)i + k];
        }
        aux_bwd_chain<F64>(cam, rec6, sums, m3, sc, q, a.cov3D_precomp ? c6 : nullptr, o);
    }
    gauss_grad_store(a, i, o);
}

// The per-Gaussian kernel of the _screen entry points (r3dgs_aux_maps_backward_screen, r3dgs_distortion_backward_screen,
// r3dgs_feature_maps_backward_screen): aux_bwd_gauss_kernel written out once more -- the same sums in the same order, the
// same chain -- with the two screen-space outputs stored beside the six, over a slab of `rows_per_slot` 32-byte rows per list
// slot (4 for the aux and distortion slabs, 4 * groups for the feature maps' geometric slab, whose seventh float is 0: its
// dL_dz is zero).  A kernel of its own, so that the kernels above keep their arguments and their bits.
// MODEL = false: a frozen model -- none of dL_dmeans3D .. dL_dcov3D is asked for, the chain behind the screen-space sums is
// not run and of the model only radii is read (the other model pointers may be NULL).
struct ScreenGaussArgs : AuxGaussArgs {
    uint32_t rows_per_slot;
    float *dL_dconic, *dL_dz;
};

template <bool F64, bool MODEL>
__global__ __launch_bounds__(64) void screen_gauss_kernel(const ScreenGaussArgs a)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= a.P) return;
    AuxGaussGrad o;
    gauss_grad_clear(o);
    AuxScreenGrad sg = {{0.f, 0.f, 0.f}, 0.f};
    if (global_ptr(a.radii)[i] > 0) {
        const uint32_t lo = run_begin(a.keys, a.R, i);
        double sums[kAuxSums];
        for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        uint32_t j = lo;
        for (; j < a.R && global_ptr(a.keys)[j] == i; j++) {   // the run, counted as it is summed
            const uint32_t slot = global_ptr(a.slots)[j];
            if (slot >= a.R) continue;
            const auto* rows = reinterpret_cast<const R3_GLOBAL float4*>(global_ptr(a.slab)) + (size_t)slot * a.rows_per_slot * 2;
            for (uint32_t q = 0; q < a.rows_per_slot; q++) {
                const float4 r0 = rows[2 * q], r1 = rows[2 * q + 1];
                sums[0] += (double)r0.x;
                sums[1] += (double)r0.y;
                sums[2] += (double)r0.z;
                sums[3] += (double)r0.w;
                sums[4] += (double)r1.x;
                sums[5] += (double)r1.y;
                sums[6] += (double)r1.z;
            }
        }
        // lost pairs to an overflowed reservation: zero sums, as in aux_bwd_gauss_kernel
        if (j - lo != global_ptr(a.tiles)[i])
            for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        Camera cam;
        for (int k = 0; k < 16; k++) {
            cam.view[k] = MODEL ? global_ptr(a.view)[k] : 0.f;
            cam.proj[k] = MODEL ? global_ptr(a.proj)[k] : 0.f;
        }
        cam.campos[0] = cam.campos[1] = cam.campos[2] = 0.f;   // (no term of this chain looks at it)
        cam.tan_fovx = a.tan_fovx;
        cam.tan_fovy = a.tan_fovy;
        cam.focal_y = a.H / (2.0f * a.tan_fovy);
        cam.focal_x = a.W / (2.0f * a.tan_fovx);
        cam.W = a.W;
        cam.H = a.H;
        cam.gx = (a.W + kTile - 1) / kTile;
        cam.gy = (a.H + kTile - 1) / kTile;
        cam.scale_modifier = a.scale_modifier;
        const GRec r = global_ptr(a.rec)[i];
        const float rec6[6] = {r.x, r.y, r.cA, r.cB, r.cC, r.op};
        float m3[3] = {0.f, 0.f, 1.f}, sc[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c6[6];
        bool precomp = false;
        if (MODEL) {
            precomp = a.cov3D_precomp != nullptr;
            for (int k = 0; k < 3; k++) m3[k] = global_ptr(a.means3D)[3 * (size_t)i + k];
            if (precomp) {
                for (int k = 0; k < 6; k++) c6[k] = global_ptr(a.cov3D_precomp)[6 * (size_t)i + k];
            } else {
                for (int k = 0; k < 3; k++) sc[k] = global_ptr(a.scales)[3 * (size_t)i + k];
                for (int k = 0; k < 4; k++) q[k] = global_ptr(a.rotations)[4 * (size_t)i + k];
            }
        }
        // (MODEL = false: everything of the chain behind the screen-space gradients is unread and the compiler drops it)
        aux_bwd_chain<F64>(cam, rec6, sums, m3, sc, q, precomp ? c6 : nullptr, o, &sg);
    }
    if (MODEL) {
        gauss_grad_store(a, i, o);
    } else if (a.dL_dmeans2D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dmeans2D) + 3 * (size_t)i;
        d[0] = o.mean2D[0];
        d[1] = o.mean2D[1];
        d[2] = 0.f;
    }
    if (a.dL_dconic) {
        R3_GLOBAL float* d = global_ptr(a.dL_dconic) + 4 * (size_t)i;
        d[0] = sg.conic[0];
        d[1] = sg.conic[1];
        d[2] = 0.f;
        d[3] = sg.conic[2];
    }
    if (a.dL_dz) global_ptr(a.dL_dz)[i] = sg.z;
}

// the workspace: the slab, then the sort's arrays and temp storage
struct AuxBwdWork {
    float* slab;
    PairSortWork sort;
    char* end;
    static AuxBwdWork carve(char* base, size_t R, size_t temp_bytes)
    {
        Carver c(base);
        AuxBwdWork w;
        w.slab = c.take<float>(R * kAuxQuads * kAuxRowFloats);
        w.sort = PairSortWork::carve(c, R, temp_bytes);
        w.end = c.p;
        return w;
    }
};

}  // namespace

// ---- the second stage, shared with the units that write the same slab (aux_bwd_stage.h) ---------------------------------
size_t aux_bwd_workspace_bytes(size_t R)
{
    return (size_t)reinterpret_cast<uintptr_t>(AuxBwdWork::carve(nullptr, R, pair_sort_temp_bytes(R)).end) + kAlign;
}

float* aux_bwd_slab(char* workspace, size_t R) { return AuxBwdWork::carve(workspace, R, 0).slab; }

void aux_bwd_zero_outputs(int P, const AuxBwdGeom& g, hipStream_t s)
{
    const size_t n = (size_t)P;
    if (g.dL_dmeans2D) R3_HIP(hipMemsetAsync(g.dL_dmeans2D, 0, sizeof(float) * 3 * n, s));
    if (g.dL_dmeans3D) R3_HIP(hipMemsetAsync(g.dL_dmeans3D, 0, sizeof(float) * 3 * n, s));
    if (g.dL_dopacity) R3_HIP(hipMemsetAsync(g.dL_dopacity, 0, sizeof(float) * n, s));
    if (g.dL_dscales) R3_HIP(hipMemsetAsync(g.dL_dscales, 0, sizeof(float) * 3 * n, s));
    if (g.dL_drotations) R3_HIP(hipMemsetAsync(g.dL_drotations, 0, sizeof(float) * 4 * n, s));
    if (g.dL_dcov3D) R3_HIP(hipMemsetAsync(g.dL_dcov3D, 0, sizeof(float) * 6 * n, s));
    if (g.dL_dconic) R3_HIP(hipMemsetAsync(g.dL_dconic, 0, sizeof(float) * 4 * n, s));
    if (g.dL_dz) R3_HIP(hipMemsetAsync(g.dL_dz, 0, sizeof(float) * n, s));
}

void aux_bwd_check_geom(const char* what, const AuxBwdGeom& g)
{
    if (g.screen_output() && !g.model_output()) {   // a frozen model (a _screen call for the camera alone): only radii is read
        if (!g.radii) throw Error(std::string(what) + ": radii must not be NULL");
        return;
    }
    if (!g.viewmatrix || !g.projmatrix || !g.means3D || !g.radii)
        throw Error(std::string(what) + ": viewmatrix, projmatrix, means3D and radii must not be NULL");
    if (!g.cov3D_precomp && (!g.scales || !g.rotations))
        throw Error(std::string(what) + ": need scales and rotations, or cov3D_precomp");
}

void launch_screen_gauss(const char* what, const PassStates& st, const PairSortWork& sort, int P, int R, int width, int height,
                         const AuxBwdGeom& in, const float* slab, uint32_t rows_per_slot, hipStream_t s)
{
    ScreenGaussArgs g = gauss_args_of<ScreenGaussArgs>(st, sort, P, R, width, height, in);
    g.slab = slab;
    g.rows_per_slot = rows_per_slot;
    g.dL_dconic = in.dL_dconic;
    g.dL_dz = in.dL_dz;
    const uint32_t gblocks = ((uint32_t)P + 63u) / 64u;
    const bool f64 = g_f64_chain.get() != 0;
    if (in.model_output()) {
        if (f64)
            hipLaunchKernelGGL((screen_gauss_kernel<true, true>), dim3(gblocks), dim3(64), 0, s, g);
        else
            hipLaunchKernelGGL((screen_gauss_kernel<false, true>), dim3(gblocks), dim3(64), 0, s, g);
    } else {   // (no double chain to select: the kernel stops at the screen-space sums)
        hipLaunchKernelGGL((screen_gauss_kernel<false, false>), dim3(gblocks), dim3(64), 0, s, g);
    }
    check_launch((std::string(what) + ", per-Gaussian chain with screen-space outputs").c_str(), s, false);
}

void aux_bwd_second_stage(const PassStates& st, int P, int R, int width, int height, const AuxBwdGeom& in, char* workspace,
                          hipStream_t s)
{
    const AuxBwdWork w = AuxBwdWork::carve(workspace, (size_t)R, pair_sort_temp_bytes((size_t)R));
    launch_pair_sort("aux maps backward", st, P, R, w.sort, s);
    if (in.screen_output()) {
        launch_screen_gauss("aux maps backward", st, w.sort, P, R, width, height, in, w.slab, kAuxQuads, s);
        return;
    }
    AuxGaussArgs g = gauss_args_of<AuxGaussArgs>(st, w.sort, P, R, width, height, in);
    g.slab = w.slab;
    const uint32_t gblocks = ((uint32_t)P + 63u) / 64u;
    if (g_f64_chain.get())
        hipLaunchKernelGGL(aux_bwd_gauss_kernel<true>, dim3(gblocks), dim3(64), 0, s, g);
    else
        hipLaunchKernelGGL(aux_bwd_gauss_kernel<false>, dim3(gblocks), dim3(64), 0, s, g);
    check_launch("aux maps backward, per-Gaussian chain", s, false);
}

}  // namespace r3

extern "C" {

size_t r3dgs_aux_maps_backward_workspace_bytes(int P, int R, int width, int height)
{
    size_t out = 0;
    r3::guarded_call([&]() {
        using namespace r3;
        check_replay_dims("aux_maps_backward_workspace_bytes", P, R, width, height);
        if (P == 0 || R == 0) return 0;
        out = aux_bwd_workspace_bytes((size_t)R);
        return 0;
    });
    return out;
}

int r3dgs_aux_maps_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                            const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                            const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                            const float* cov3D_precomp, const int* radii, const float* dL_ddepth, const float* dL_dalpha,
                            const float* dL_dmedian, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity,
                            float* dL_dscales, float* dL_drotations, float* dL_dcov3D, char* workspace, void* stream)
{
    return r3dgs_aux_maps_backward_screen(P, R, width, height, geom_buffer, binning_buffer, image_buffer, viewmatrix, projmatrix,
                                          tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations, cov3D_precomp, radii,
                                          dL_ddepth, dL_dalpha, dL_dmedian, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales,
                                          dL_drotations, dL_dcov3D, nullptr, nullptr, workspace, stream);
}

int r3dgs_aux_maps_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                   char* image_buffer, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                                   float tan_fovy, const float* means3D, const float* scales, float scale_modifier,
                                   const float* rotations, const float* cov3D_precomp, const int* radii, const float* dL_ddepth,
                                   const float* dL_dalpha, const float* dL_dmedian, float* dL_dmeans2D, float* dL_dmeans3D,
                                   float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                                   float* dL_dconic, float* dL_dz, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        // (without the two screen-space outputs this is r3dgs_aux_maps_backward itself, message for message)
        const char* const what = dL_dconic || dL_dz ? "aux_maps_backward_screen" : "aux_maps_backward";
        const AuxBwdGeom geom = {viewmatrix, projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                 cov3D_precomp, radii, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D,
                                 dL_dconic, dL_dz};
        const auto w = replay_bwd_open(
            what, P, R, width, height, {geom_buffer, binning_buffer, image_buffer},
            dL_ddepth || dL_dalpha || dL_dmedian, geom, nullptr, 0, workspace, s,
            [&](const char* what) { check_replay_dims(what, P, R, width, height); },
            [&] { aux_bwd_check_geom(what, geom); });
        if (!w) return 0;
        const PassStates& st = w->st;
        const AuxBwdArgs a = {walk_args_of(st, w->grid, P, R, width, height), dL_ddepth, dL_dalpha, dL_dmedian,
                              aux_bwd_slab(workspace, (size_t)R)};
        hipLaunchKernelGGL(aux_bwd_pixel_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("aux maps backward, pixel pass", s, false);
        aux_bwd_second_stage(st, P, R, width, height, geom, workspace, s);
        return 0;
    });
}

}  // extern "C"
