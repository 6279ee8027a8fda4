// importance.hip -- per-Gaussian blend-contribution scores of a view (include/r3dgs_importance.h; the arithmetic is
// importance_math.h), gfx950: the sum, the maximum and the count of the blend weights w = alpha * T a Gaussian had over the
// pixels, under an optional pixel weight map.  A replay pass (DESIGN.md "Replay passes"): it reads the three state blobs and
// writes only the caller's outputs and workspace.
//
// Four launches on the caller's stream (the route of aux_bwd.hip; no host wait, no allocation, no atomics):
//   1. imp_walk_kernel -- the walk (replay_walk.h) front to back with T running forward from 1 (only T_before is needed:
//      nothing is recovered by division).  Per entry some lane counted, three wave reductions in a fixed lane order: the sum
//      of m * w and the maximum of w (the mirror order, importance_math.h imp_tree_sum / imp_tree_max) and the count (ballot
//      and popcount).  Per chunk, lane j stores the 16-byte row of entry j -- or the zero row for an entry whose pre-test
//      failed or that no lane counted -- at rows[list slot * 4 + quadrant]; the slots of the list behind the walk get zero
//      rows.  The step is the forward's own, and build.py compiles this unit with blend.hip's flags: the walk's final T and
//      last contributor are the forward's bit for bit (T_check / n_check).
//   2, 3. the (Gaussian id, list slot) keys and their stable sort by id (pair_sort.h).
//   4. imp_gauss_kernel -- one lane per Gaussian: its run of the sorted keys, its rows added in sorted order (slot
//      ascending, quadrant 0..3): sum in double, max in float, count in integers; the overflow rule and `accumulate`
//      (importance_math.h imp_fold); every row of every output is written.
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
// Workspace per pair: 4 x 16 B rows + 16 B of keys and slots = 80 bytes, plus rocPRIM's temp storage.
#include <string>

#include "../../include/r3dgs_importance.h"
#include "importance_math.h"
#include "common.h"
#include "pair_sort.h"
#include "pass_driver.h"
#include "replay_walk.h"

namespace r3 {

namespace {

static_assert(sizeof(ImpRow) == 16, "one 16-byte store per row");

struct ImpArgs : WalkArgs {
    const float* weight;     // [H*W] or nullptr (ones)
    ImpRow* rows;            // [R][4]
    float* T_check;
    uint32_t* n_check;
};

__global__ __launch_bounds__(64) void imp_walk_kernel(const ImpArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    __shared__ uint4 s_out[kWalkChunk];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const WalkSpan sp = load_walk_span(a, q);
    const uint32_t first = sp.first, len = sp.len;
    const float pxf = q.pxf, pyf = q.pyf;
    R3_GLOBAL uint4* const rows = reinterpret_cast<R3_GLOBAL uint4*>(global_ptr(a.rows));
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // the slots behind the walk: zero rows
    for (uint32_t k = len + (uint32_t)lane; k < sp.list_len; k += kWalkChunk)
        rows[(size_t)(first + k) * kImpQuads + (size_t)q.quad] = zero4;

    uint32_t n = 0u;
    float m = 0.f;
    if (q.inside) {
        n = global_ptr(a.n_contrib)[q.pix];
        m = a.weight ? global_ptr(a.weight)[q.pix] : 1.0f;
    }
    FwdPix p;
    fwd_pix_init(p, q.inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    WalkGather nx = gather_rec(a.point_list + first, a.rec, a.P, (uint32_t)lane, len);
    for (uint32_t base = 0u; base < len; base += kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, 0.f, __uint_as_float(base + (uint32_t)lane + 1u));
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        nx = gather_rec(a.point_list + first, a.rec, a.P, base + kWalkChunk + (uint32_t)lane, len);
        unsigned long long counted = 0ull;   // wave-uniform: entries of this chunk some lane counted
        while (mask) {   // front to back: lowest set bit first
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            float w, mw;
            const bool hit = imp_step(load_splat(s_rec[j]), pxf, pyf, load_pos1(s_rec[j]), n, m, p, &w, &mw);
            const unsigned long long hits = __ballot(hit);
            if (hits != 0ull) {
                const float rs = wave_sum_mirror(mw), rm = wave_max_mirror(w);
                if (lane == 0) s_out[j] = make_uint4(__float_as_uint(rs), __float_as_uint(rm), (uint32_t)__builtin_popcountll(hits), 0u);
                counted |= 1ull << j;
            }
        }
        __syncthreads();
        if (base + (uint32_t)lane < len) {
            uint4 o = s_out[lane];
            if (!((counted >> lane) & 1ull)) o = zero4;
            rows[(size_t)(first + base + (uint32_t)lane) * kImpQuads + (size_t)q.quad] = o;
        }
    }
    if (q.inside) {
        if (a.T_check) global_ptr(a.T_check)[q.pix] = fwd_pix_T(p);
        if (a.n_check) global_ptr(a.n_check)[q.pix] = p.last;
    }
}

struct ImpSumArgs {
    const uint32_t* tiles;   // [P] tiles_touched: the pairs the forward wanted for the Gaussian
    const uint32_t* keys;    // [R] sorted ids
    const uint32_t* slots;   // [R] their list slots
    const ImpRow* rows;
    uint32_t P, R;
    int accumulate;
    double* sum;
    float* max;
    long long* count;
    int* views;
};

__global__ __launch_bounds__(256) void imp_gauss_kernel(const ImpSumArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.P) return;
    uint32_t count;
    const uint32_t lo = run_of(a.keys, a.R, i, &count);
    ImpScore view;
    imp_score_clear(view);
    for (uint32_t j = lo; j < lo + count; j++) {
        const uint32_t slot = global_ptr(a.slots)[j];
        if (slot >= a.R) continue;
        const auto* rows = reinterpret_cast<const R3_GLOBAL uint4*>(global_ptr(a.rows)) + (size_t)slot * kImpQuads;
#pragma unroll
        for (int q = 0; q < kImpQuads; q++) {
            const uint4 r = rows[q];
            imp_add_row(view, __uint_as_float(r.x), __uint_as_float(r.y), r.z);
        }
    }
    ImpScore held;
    imp_score_clear(held);
    if (a.accumulate) {
        if (a.sum) held.sum = global_ptr(a.sum)[i];
        if (a.max) held.max = global_ptr(a.max)[i];
        if (a.count) held.count = global_ptr(a.count)[i];
        if (a.views) held.views = global_ptr(a.views)[i];
    }
    const ImpScore o = imp_fold(view, imp_run_complete(count, global_ptr(a.tiles)[i]), a.accumulate != 0, held);
    if (a.sum) global_ptr(a.sum)[i] = o.sum;
    if (a.max) global_ptr(a.max)[i] = o.max;
    if (a.count) global_ptr(a.count)[i] = o.count;
    if (a.views) global_ptr(a.views)[i] = o.views;
}

// the workspace: the rows, then the sort's arrays and temp storage
struct ImpWork {
    ImpRow* rows;
    PairSortWork sort;
    char* end;
    static ImpWork carve(char* base, size_t R, size_t temp_bytes)
    {
        Carver c(base);
        ImpWork w;
        w.rows = c.take<ImpRow>(R * kImpQuads);
        w.sort = PairSortWork::carve(c, R, temp_bytes);
        w.end = c.p;
        return w;
    }
};

}  // namespace

}  // namespace r3

extern "C" {

size_t r3dgs_contribution_scores_workspace_bytes(int P, int R, int width, int height)
{
    size_t out = 0;
    r3::guarded_call([&]() {
        using namespace r3;
        check_replay_dims("contribution_scores_workspace_bytes", P, R, width, height);
        if (P == 0 || R == 0) return 0;
        out = (size_t)reinterpret_cast<uintptr_t>(ImpWork::carve(nullptr, (size_t)R, pair_sort_temp_bytes((size_t)R)).end) + kAlign;
        return 0;
    });
    return out;
}

int r3dgs_contribution_scores(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                              const float* pixel_weight, double* score_sum, float* score_max, long long* score_count,
                              int* score_views, int accumulate, float* T_check, unsigned* n_check, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_replay_dims("contribution_scores", P, R, width, height);
        if (accumulate != 0 && accumulate != 1)
            throw Error("contribution_scores: accumulate must be 0 or 1, got " + std::to_string(accumulate));
        const TileGrid grid = replay_grid("contribution_scores", width, height);
        const size_t N = (size_t)width * height;
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk, the blobs are not read
            const size_t n = (size_t)P;
            if (!accumulate && n) {
                if (score_sum) R3_HIP(hipMemsetAsync(score_sum, 0, sizeof(double) * n, s));
                if (score_max) R3_HIP(hipMemsetAsync(score_max, 0, sizeof(float) * n, s));
                if (score_count) R3_HIP(hipMemsetAsync(score_count, 0, sizeof(long long) * n, s));
                if (score_views) R3_HIP(hipMemsetAsync(score_views, 0, sizeof(int) * n, s));
            }
            // T = 1 everywhere: nothing was blended
            if (T_check) R3_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T_check), 0x3f800000, N, s));
            if (n_check) R3_HIP(hipMemsetAsync(n_check, 0, sizeof(unsigned) * N, s));
            return 0;
        }
        const bool scores = score_sum || score_max || score_count || score_views;
        if (!scores && !T_check && !n_check) return 0;
        const PassStates st = replay_states("contribution_scores", P, R, width, height, {geom_buffer, binning_buffer, image_buffer});
        if (!workspace) throw Error("contribution_scores: the workspace must not be NULL");
        const ImpWork w = ImpWork::carve(workspace, (size_t)R, pair_sort_temp_bytes((size_t)R));

        const ImpArgs a = {walk_args_of(st, grid, P, R, width, height), pixel_weight, w.rows, T_check, n_check};
        hipLaunchKernelGGL(imp_walk_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("contribution scores, walk", s, false);
        if (!scores) return 0;
        launch_pair_sort("contribution scores", st, P, R, w.sort, s);

        const ImpSumArgs g = {st.geom.tiles, w.sort.keys_out, w.sort.slots_out, w.rows, (uint32_t)P, (uint32_t)R, accumulate,
                              score_sum, score_max, score_count, score_views};
        hipLaunchKernelGGL(imp_gauss_kernel, dim3(((uint32_t)P + 255u) / 256u), dim3(256), 0, s, g);
        check_launch("contribution scores, per-Gaussian fold", s, false);
        return 0;
    });
}

}  // extern "C"
