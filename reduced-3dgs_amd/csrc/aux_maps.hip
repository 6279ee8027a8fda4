// aux_maps.hip -- expected depth, accumulated opacity and median depth per pixel, replayed from the state a forward pass
// left (include/r3dgs_aux.h; the arithmetic is aux_math.h), gfx950.
//
// A replay pass (DESIGN.md "Replay passes"; the walk's shared part is replay_walk.h): the forward blend's structure
// (blend.hip) without the colour.  What is particular to this unit:
//   * lane j stages, beside the record of entry j, its depth word (GeomState::depth_key, the float bits of the view depth)
//     and its 1-based list position: a pixel looks at no entry behind its own n_contrib;
//   * the per-(pixel, entry) step is the forward's own (fwd_alpha / fwd_apply through aux_math.h), and build.py compiles this
//     unit with blend.hip's flags: T after every entry, the final T and the last contributor are the forward's bit for bit
//     (r3dgs_aux_maps hands them out as T_check / n_check and the tests hold them to final_T / n_contrib).
// It writes only the caller's output arrays -- the blobs stay as the forward left them, for the backward.  Plain vector
// stores, no atomics; 2 KB of LDS per workgroup.
#include <string>

#include "../../include/r3dgs_aux.h"
#include "aux_math.h"
#include "common.h"
#include "pass_driver.h"
#include "replay_walk.h"

namespace r3 {

namespace {

constexpr int kAuxBatch = 4;   // entries whose alphas are evaluated side by side before they are composited in order

struct AuxArgs : WalkArgs {
    float* depth;
    float* alpha;
    float* median;
    float* T_check;
    uint32_t* n_check;
};

__global__ __launch_bounds__(64) void aux_maps_kernel(const AuxArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const WalkSpan sp = load_walk_span(a, q);
    const uint32_t first = sp.first, end = sp.first + sp.len;
    const float pxf = q.pxf, pyf = q.pyf;
    const uint32_t n = q.inside ? global_ptr(a.n_contrib)[q.pix] : 0u;
    AuxPix p;
    aux_pix_init(p, q.inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    uint32_t nxz = 0u;
    auto gather = [&](uint32_t idx) {
        const WalkGather g = gather_rec(a.point_list, a.rec, a.P, idx, end);
        if (g.have) nxz = global_ptr(a.depth_key)[g.id];
        return g;
    };
    WalkGather nx = gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, __uint_as_float(nxz), __uint_as_float(base - first + (uint32_t)lane + 1u));
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        nx = gather(base + kWalkChunk + (uint32_t)lane);
        for (int left = __builtin_popcountll(mask); left >= kAuxBatch; left -= kAuxBatch) {
            QSplat s4[kAuxBatch];
            uint32_t pos1[kAuxBatch];
            float al[kAuxBatch];
            bool inb[kAuxBatch];
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                s4[i] = load_splat_z(s_rec[j]);
                pos1[i] = load_pos1(s_rec[j]);
            }
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) al[i] = fwd_alpha(s4[i], pxf, pyf, &inb[i]);
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) aux_apply(s4[i], al[i], inb[i], pos1[i], n, p);
        }
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            aux_step(load_splat_z(s_rec[j]), pxf, pyf, load_pos1(s_rec[j]), n, p);
        }
    }
    if (q.inside) {
        const size_t pix = q.pix;
        if (a.depth) global_ptr(a.depth)[pix] = aux_depth(p);
        if (a.alpha) global_ptr(a.alpha)[pix] = 1.0f - global_ptr(a.final_T)[pix];
        if (a.median) global_ptr(a.median)[pix] = p.median;
        if (a.T_check) global_ptr(a.T_check)[pix] = fwd_pix_T(p.f);
        if (a.n_check) global_ptr(a.n_check)[pix] = p.f.last;
    }
}

}  // namespace

}  // namespace r3

extern "C" {

int r3dgs_aux_maps(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                   float* depth, float* alpha, float* median_depth, float* T_check, unsigned* n_check, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_replay_dims("aux_maps", P, R, width, height);
        const TileGrid grid = replay_grid("aux_maps", width, height);
        const size_t N = (size_t)width * height;
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            float* const maps[4] = {depth, alpha, median_depth, T_check};
            for (float* m : maps)
                if (m) R3_HIP(hipMemsetAsync(m, 0, sizeof(float) * N, s));
            if (n_check) R3_HIP(hipMemsetAsync(n_check, 0, sizeof(uint32_t) * N, s));
            return 0;
        }
        // (the arrays read here lie in front of the geometry blob's temp storage and of its optional tail: their offsets
        // are those of every forward's carve, lean or full)
        const PassStates st = replay_states("aux_maps", P, R, width, height, {geom_buffer, binning_buffer, image_buffer});
        if (!depth && !alpha && !median_depth && !T_check && !n_check) return 0;
        const AuxArgs a = {walk_args_of(st, grid, P, R, width, height), depth, alpha, median_depth, T_check, n_check};
        hipLaunchKernelGGL(aux_maps_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("aux maps", s, false);
        return 0;
    });
}

}  // extern "C"
