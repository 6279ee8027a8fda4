// distortion.hip -- the depth-distortion map (the squared form of the 2DGS regulariser) and the pixel pass of the gradients
// through it, replayed from the state a forward pass left (include/r3dgs_distortion.h; the arithmetic is distortion_math.h),
// gfx950.  Two replay passes (DESIGN.md "Replay passes"; the walk's shared part is replay_walk.h): they read the three state
// blobs and write only the caller's outputs and workspace.
//
//   dist_map_kernel -- the walk front to back.  The staging lane maps the entry's view depth and shifts it by the mapped
//     depth of the tile's first list entry (once per entry, not per pixel); the per-(pixel, entry) step is the forward's own
//     (fwd_alpha / fwd_apply through distortion_math.h), so the weights are the forward's.  Writes distortion [H*W] and, when
//     asked, the shifted moments S1, S2 [2, H*W].
//   dist_bwd_pixel_kernel -- the walk back to front with T recovered from final_T by division; the step is the backward
//     blend's on a splat of colour c_k (three FMAs per lane from the broadcast mapped depth) under the pixel gradient g.  It
//     writes aux_bwd's slab rows (aux_bwd_stage.h) and aux_bwd.hip's second stage (keys, stable sort, per-Gaussian double
//     sums, chain) does the rest.
// No atomics, no host wait, no allocation, no scratch; the order of every sum is fixed by the data alone.  build.py compiles
// this unit with blend.hip's flags.
#include <string>

#include "../../include/r3dgs_distortion.h"
#include "aux_bwd_stage.h"
#include "common.h"
#include "distortion_math.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kDistBatch = 4;   // entries whose alphas are evaluated side by side before they are composited in order

// the staged record's own words: b.z the shifted mapped depth; b.w forward: the 1-based list position, backward: dm/dz
struct DistArgs : WalkArgs {
    float near, far;
    float* distortion;       // forward outputs (either may be nullptr)
    float* moments;
    const float* g;          // backward inputs
    const float* saved;
    float* slab;             // backward output: [R][4][8]
};

// The depth mapping of a tile: the reference is the view depth of the first entry of its list (1 where the list is empty
// or names no Gaussian: nothing is blended there).  A function of the forward's state alone -- both passes call this.
__device__ __forceinline__ DepthMap tile_depth_map(const DistArgs& a, uint2 range)
{
    float z_ref = 1.0f;
    if (range.y > range.x && range.x < a.R) {
        const uint32_t id = global_ptr(a.point_list)[range.x];
        if (id < a.P) z_ref = __uint_as_float(global_ptr(a.depth_key)[id]);
    }
    return depth_map_of(a.near, a.far, z_ref);
}

__global__ __launch_bounds__(64) void dist_map_kernel(const DistArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const uint2 range = global_ptr(a.ranges)[q.tile];   // (also the depth mapping's)
    const WalkSpan sp = walk_span(range, global_ptr(a.quad_depth)[q.tile * 4u + (uint32_t)q.quad], a.R);
    const uint32_t first = sp.first, end = sp.first + sp.len;
    const float pxf = q.pxf, pyf = q.pyf;
    const size_t N = (size_t)a.W * (size_t)a.H;
    const uint32_t n = q.inside ? global_ptr(a.n_contrib)[q.pix] : 0u;
    const DepthMap dm = tile_depth_map(a, range);
    DistPix p;
    dist_pix_init(p, q.inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float nxm = 0.f;
    auto gather = [&](uint32_t idx) {
        const WalkGather g = gather_rec(a.point_list, a.rec, a.P, idx, end);
        if (g.have) nxm = mapped_depth_shifted(dm, __uint_as_float(global_ptr(a.depth_key)[g.id]));
        return g;
    };
    WalkGather nx = gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, nxm, __uint_as_float(base - first + (uint32_t)lane + 1u));
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        nx = gather(base + kWalkChunk + (uint32_t)lane);
        for (int left = __builtin_popcountll(mask); left >= kDistBatch; left -= kDistBatch) {
            QSplat s4[kDistBatch];
            uint32_t pos1[kDistBatch];
            float al[kDistBatch];
            bool inb[kDistBatch];
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                s4[i] = load_splat_z(s_rec[j]);
                pos1[i] = load_pos1(s_rec[j]);
            }
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) al[i] = fwd_alpha(s4[i], pxf, pyf, &inb[i]);
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) dist_apply(s4[i], al[i], inb[i], pos1[i], n, p);
        }
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            dist_step(load_splat_z(s_rec[j]), pxf, pyf, load_pos1(s_rec[j]), n, p);
        }
    }
    if (q.inside) {
        if (a.distortion) global_ptr(a.distortion)[q.pix] = dist_value(p);
        if (a.moments) {
            global_ptr(a.moments)[q.pix] = dist_moment1(p);
            global_ptr(a.moments)[N + q.pix] = dist_moment2(p);
        }
    }
}

__global__ __launch_bounds__(64) void dist_bwd_pixel_kernel(const DistArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    __shared__ float4 s_out[kWalkChunk][2];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const uint2 range = global_ptr(a.ranges)[q.tile];   // (also the depth mapping's)
    const WalkSpan sp = walk_span(range, global_ptr(a.quad_depth)[q.tile * 4u + (uint32_t)q.quad], a.R);
    const uint32_t len = sp.len;
    const float pxf = q.pxf, pyf = q.pyf;
    const size_t N = (size_t)a.W * (size_t)a.H;
    R3_GLOBAL float4* const rows = reinterpret_cast<R3_GLOBAL float4*>(global_ptr(a.slab));
    slab_zero_behind(rows, sp, q.quad, lane);
    if (len == 0u) return;

    const DepthMap dm = tile_depth_map(a, range);
    BwdPix p;
    DistTotals tot;
    tot.A = tot.S1 = tot.S2 = 0.f;
    {
        float T = 1.f, g = 0.f;
        uint32_t n = 0u;
        if (q.inside) {
            T = global_ptr(a.final_T)[q.pix];
            n = global_ptr(a.n_contrib)[q.pix];
            g = global_ptr(a.g)[q.pix];
            tot.A = 1.0f - T;
            tot.S1 = global_ptr(a.saved)[q.pix];
            tot.S2 = global_ptr(a.saved)[N + q.pix];
        }
        dist_bwd_pix_init(p, q.inside, T, n, g);
    }

    // software pipeline: the records of the next (shallower) chunk are gathered into registers while a chunk is walked
    float nxm = 0.f, nxd = 0.f;
    auto gather = [&](uint32_t k) {   // k: position in the list
        const WalkGather g = gather_rec(a.point_list + sp.first, a.rec, a.P, k, len);
        if (g.have) {
            const float z = __uint_as_float(global_ptr(a.depth_key)[g.id]);
            nxm = mapped_depth_shifted(dm, z);
            nxd = mapped_depth_dz(dm, z);
        }
        return g;
    };
    const uint32_t cfirst = ((len - 1u) / kWalkChunk) * kWalkChunk;
    WalkGather nx = gather(cfirst + (uint32_t)lane);
    SplatSums sg;
    aux_sums_clear(sg);
    for (uint32_t cbase = cfirst;; cbase -= kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, nxm, nxd);
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        if (cbase >= kWalkChunk) nx = gather(cbase - kWalkChunk + (uint32_t)lane);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk some lane blended
        while (mask) {   // back to front: highest set bit first
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const QSplat s = load_splat_z(s_rec[j]);
            const float dmdz = s_rec[j].b.w;
            BwdEval e;
            const bool valid = bwd_test(s, pxf, pyf, cbase + (uint32_t)j, p, e);
            if (valid) dist_bwd_apply(s, dmdz, e, p, tot, sg);
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

void check_call(const char* what, int P, int R, int width, int height, float near, float far)
{
    check_replay_dims(what, P, R, width, height);
    if (!depth_map_valid(near, far))
        throw Error(std::string(what) + ": need near = far = 0 (the linear mapping) or 0 < near < far, got near = " +
                    std::to_string(near) + ", far = " + std::to_string(far));
}

DistArgs args_of(const PassStates& st, int P, int R, int width, int height, const TileGrid& grid, float near, float far)
{
    return {walk_args_of(st, grid, P, R, width, height), near, far, nullptr, nullptr, nullptr, nullptr, nullptr};
}

}  // namespace

}  // namespace r3

extern "C" {

int r3dgs_distortion_map(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                         float near, float far, float* distortion, float* saved_moments, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_call("distortion_map", P, R, width, height, near, far);
        const TileGrid grid = replay_grid("distortion_map", width, height);
        const size_t N = (size_t)width * height;
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            if (distortion) R3_HIP(hipMemsetAsync(distortion, 0, sizeof(float) * N, s));
            if (saved_moments) R3_HIP(hipMemsetAsync(saved_moments, 0, sizeof(float) * 2 * N, s));
            return 0;
        }
        const PassStates st = replay_states("distortion_map", P, R, width, height, {geom_buffer, binning_buffer, image_buffer});
        if (!distortion && !saved_moments) return 0;
        DistArgs a = args_of(st, P, R, width, height, grid, near, far);
        a.distortion = distortion;
        a.moments = saved_moments;
        hipLaunchKernelGGL(dist_map_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("distortion map", s, false);
        return 0;
    });
}

size_t r3dgs_distortion_map_backward_workspace_bytes(int P, int R, int width, int height)
{
    size_t out = 0;
    r3::guarded_call([&]() {
        using namespace r3;
        check_call("distortion_map_backward_workspace_bytes", P, R, width, height, 0.f, 0.f);
        if (P == 0 || R == 0) return 0;
        out = aux_bwd_workspace_bytes((size_t)R);
        return 0;
    });
    return out;
}

int r3dgs_distortion_map_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                  char* image_buffer, float near, float far, const float* viewmatrix, const float* projmatrix,
                                  float tan_fovx, float tan_fovy, const float* means3D, const float* scales,
                                  float scale_modifier, const float* rotations, const float* cov3D_precomp, const int* radii,
                                  const float* dL_ddistortion, const float* saved_moments, float* dL_dmeans2D,
                                  float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                                  float* dL_dcov3D, char* workspace, void* stream)
{
    return r3dgs_distortion_backward_screen(P, R, width, height, geom_buffer, binning_buffer, image_buffer, near, far, viewmatrix,
                                            projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                            cov3D_precomp, radii, dL_ddistortion, saved_moments, dL_dmeans2D, dL_dmeans3D,
                                            dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, nullptr, nullptr, workspace, stream);
}

int r3dgs_distortion_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                     char* image_buffer, float near, float far, const float* viewmatrix, const float* projmatrix,
                                     float tan_fovx, float tan_fovy, const float* means3D, const float* scales,
                                     float scale_modifier, const float* rotations, const float* cov3D_precomp, const int* radii,
                                     const float* dL_ddistortion, const float* saved_moments, float* dL_dmeans2D,
                                     float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales, float* dL_drotations,
                                     float* dL_dcov3D, float* dL_dconic, float* dL_dz, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        // (without the two screen-space outputs this is r3dgs_distortion_map_backward itself, message for message)
        const std::string name = dL_dconic || dL_dz ? "distortion_backward_screen" : "distortion_map_backward";
        const AuxBwdGeom geom = {viewmatrix, projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                 cov3D_precomp, radii, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D,
                                 dL_dconic, dL_dz};
        const auto w = replay_bwd_open(
            name.c_str(), P, R, width, height, {geom_buffer, binning_buffer, image_buffer}, dL_ddistortion != nullptr,
            geom, nullptr, 0, workspace, s, [&](const char* what) { check_call(what, P, R, width, height, near, far); },
            [&] {
                if (!saved_moments) throw Error(name + ": saved_moments must not be NULL");
                aux_bwd_check_geom(name.c_str(), geom);
            });
        if (!w) return 0;
        const PassStates& st = w->st;
        DistArgs a = args_of(st, P, R, width, height, w->grid, near, far);
        a.g = dL_ddistortion;
        a.saved = saved_moments;
        a.slab = aux_bwd_slab(workspace, (size_t)R);
        hipLaunchKernelGGL(dist_bwd_pixel_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("distortion map backward, pixel pass", s, false);
        aux_bwd_second_stage(st, P, R, width, height, geom, workspace, s);
        return 0;
    });
}

}  // extern "C"
