// importance.hip -- per-Gaussian blend-contribution scores of a view (include/r3dgs_importance.h; the arithmetic is
// importance_math.h), gfx950: the sum, the maximum and the count of the blend weights w = alpha * T a Gaussian had over the
// pixels, under an optional pixel weight map.  A pass of its own behind any forward, like aux_maps.hip / aux_bwd.hip /
// feature_maps.hip: it reads the three state blobs and writes only the caller's outputs and workspace.
//
// Four launches on the caller's stream (the route of aux_bwd.hip; no host wait, no allocation, no atomics):
//   1. imp_walk_kernel -- aux_maps_kernel's shape: one 64-lane wave per 8x8 quadrant of a tile, one pixel per lane; the
//      tile's list is fetched 64 entries at a time, one chunk ahead of its use, and parked in LDS as 32-byte records; the
//      walk runs front to back with T running forward from 1 (only T_before is needed: nothing is recovered by division) and
//      ends at the quadrant's deepest contributor (ImageState::quad_depth); lane j runs the forward's region pre-test for
//      entry j.  Per entry some lane counted, three wave reductions in a fixed lane order: the sum of m * w and the maximum of
//      w (DPP row steps, then two cross-row steps; both partners of every step combine the same two numbers) and the count
//      (ballot and popcount).  Per chunk, lane j stores the 16-byte row of entry j -- or the zero row for an entry whose
//      pre-test failed or that no lane counted -- at rows[list slot * 4 + quadrant]; the slots of the list behind the walk
//      get zero rows.  Every (slot < num_pairs, quadrant) row is written in every call, by exactly one wave: the slab needs
//      no clearing.  The step is the forward's own, and build.py compiles this unit with blend.hip's flags: the walk's final
//      T and last contributor are the forward's bit for bit (T_check / n_check).
//   2. imp_keys_kernel, 3. a stable rocPRIM radix sort of (Gaussian id, list slot) by id, as in feature_maps.hip.
//   4. imp_gauss_kernel -- one lane per Gaussian: its run of the sorted keys by binary search, its rows added in sorted
//      order (slot ascending, quadrant 0..3): sum in double, max in float, count in integers; the overflow rule and
//      `accumulate` (importance_math.h imp_fold); every row of every output is written.
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
// Workspace per pair: 4 x 16 B rows + 16 B of keys and slots = 80 bytes, plus rocPRIM's temp storage.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "../../include/r3dgs_importance.h"
#include "importance_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kChunk = 64;

static_assert(sizeof(ImpRow) == 16, "one 16-byte store per row");

struct ImpRec {   // 32 B: a staged list entry
    float4 a;     // x, y, qa, qb
    float4 b;     // qc, op, unused, 1-based list position (bits)
};

__device__ __forceinline__ QSplat load_splat(const ImpRec& r) { return imp_splat(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y); }

// consecutive logical ids on one XCD, as the forward blend places its tiles (speed only)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

#define R3_IMP_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))

// Full-wave reductions, the result in every lane, in the order of importance_math.h imp_tree_sum / imp_tree_max: every step
// is an exchange between two partners (lane ^ 1, lane ^ 2, the mirror of a half row, the mirror of a row -- after the first
// two steps a quad holds one value, so the mirrors pair quad with quad and half row with half row -- then lane ^ 16 and
// lane ^ 32), both of which combine the same two numbers.
__device__ __forceinline__ float wave_sum(float v)
{
    v += R3_IMP_DPP(v, 0xb1);    // quad_perm [1,0,3,2]
    v += R3_IMP_DPP(v, 0x4e);    // quad_perm [2,3,0,1]
    v += R3_IMP_DPP(v, 0x141);   // row_half_mirror
    v += R3_IMP_DPP(v, 0x140);   // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
    v = fmaxf(v, R3_IMP_DPP(v, 0xb1));
    v = fmaxf(v, R3_IMP_DPP(v, 0x4e));
    v = fmaxf(v, R3_IMP_DPP(v, 0x141));
    v = fmaxf(v, R3_IMP_DPP(v, 0x140));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

struct ImpArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    const float* weight;     // [H*W] or nullptr (ones)
    int W, H, gx;
    uint32_t nblocks;
    uint32_t P, R;           // bounds of rec and of point_list / the rows
    ImpRow* rows;            // [R][4]
    float* T_check;
    uint32_t* n_check;
};

__global__ __launch_bounds__(64) void imp_walk_kernel(const ImpArgs a)
{
    __shared__ ImpRec s_rec[kChunk];
    __shared__ uint4 s_out[kChunk];
    const int lane = threadIdx.x;
    const uint32_t wg = xcd_remap(blockIdx.x, a.nblocks);
    const uint32_t tile = wg >> 2;
    const int quad = (int)(wg & 3u);
    const int tile_x = (int)(tile % (uint32_t)a.gx), tile_y = (int)(tile / (uint32_t)a.gx);
    const float qx0 = (float)(tile_x * kTile + (quad & 1) * 8), qy0 = (float)(tile_y * kTile + (quad >> 1) * 8);
    const int px = tile_x * kTile + (quad & 1) * 8 + (lane & 7), py = tile_y * kTile + (quad >> 1) * 8 + (lane >> 3);
    const float pxf = (float)px, pyf = (float)py;
    const bool inside = px < a.W && py < a.H;
    const size_t pix = (size_t)a.W * (size_t)py + (size_t)px;

    const uint2 range = global_ptr(a.ranges)[tile];
    // the list inside the blob, and the part of it this quadrant walks: up to its deepest contributor
    const uint32_t full = range.y > range.x ? range.y - range.x : 0u;
    const uint32_t first = min(range.x, a.R);
    const uint32_t list_len = min(full, a.R - first);
    const uint32_t len = min(list_len, global_ptr(a.quad_depth)[tile * 4u + (uint32_t)quad]);
    R3_GLOBAL uint4* const rows = reinterpret_cast<R3_GLOBAL uint4*>(global_ptr(a.rows));
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // the slots behind the walk: zero rows
    for (uint32_t k = len + (uint32_t)lane; k < list_len; k += kChunk) rows[(size_t)(first + k) * kImpQuads + (size_t)quad] = zero4;

    uint32_t n = 0u;
    float m = 0.f;
    if (inside) {
        n = global_ptr(a.n_contrib)[pix];
        m = a.weight ? global_ptr(a.weight)[pix] : 1.0f;
    }
    FwdPix p;
    fwd_pix_init(p, inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float4 nxa = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 nxb = make_float2(0.f, 0.f);
    bool nxhave = false;
    auto gather = [&](uint32_t k) {   // k: position in the list
        nxhave = false;
        if (k < len) {
            const uint32_t id = global_ptr(a.point_list)[first + k];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                nxhave = true;
            }
        }
    };
    gather((uint32_t)lane);
    for (uint32_t base = 0u; base < len; base += kChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, 0.f, __uint_as_float(base + (uint32_t)lane + 1u));
        unsigned long long mask;
        {   // the forward's region pre-test, by the lane that holds the entry
            Splat mine;
            mine.x = nxa.x;
            mine.y = nxa.y;
            mine.cA = nxa.z;
            mine.cB = nxa.w;
            mine.cC = nxb.x;
            mine.op = nxb.y;
            mine.r = mine.g = mine.b = 0.f;
            mask = __ballot(nxhave && region_may_contribute(mine, qx0, qx0 + 7.f, qy0, qy0 + 7.f));
        }
        __syncthreads();
        gather(base + kChunk + (uint32_t)lane);
        unsigned long long counted = 0ull;   // wave-uniform: entries of this chunk some lane counted
        while (mask) {   // front to back: lowest set bit first
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            float w, mw;
            const bool hit = imp_step(load_splat(s_rec[j]), pxf, pyf, __float_as_uint(s_rec[j].b.w), n, m, p, &w, &mw);
            const unsigned long long hits = __ballot(hit);
            if (hits != 0ull) {
                const float rs = wave_sum(mw), rm = wave_max(w);
                if (lane == 0) s_out[j] = make_uint4(__float_as_uint(rs), __float_as_uint(rm), (uint32_t)__builtin_popcountll(hits), 0u);
                counted |= 1ull << j;
            }
        }
        __syncthreads();
        if (base + (uint32_t)lane < len) {
            uint4 o = s_out[lane];
            if (!((counted >> lane) & 1ull)) o = zero4;
            rows[(size_t)(first + base + (uint32_t)lane) * kImpQuads + (size_t)quad] = o;
        }
    }
    if (inside) {
        if (a.T_check) global_ptr(a.T_check)[pix] = fwd_pix_T(p);
        if (a.n_check) global_ptr(a.n_check)[pix] = p.last;
    }
}

// (Gaussian id, list slot) per slot of the pair capacity
__global__ __launch_bounds__(256) void imp_keys_kernel(const GeomHeader* hdr, const uint32_t* point_list, uint32_t P, uint32_t R,
                                                       uint32_t* keys, uint32_t* slots)
{
    const uint32_t num_pairs = min(global_ptr(hdr)->num_pairs, R);
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < R; e += gridDim.x * 256u) {
        uint32_t key = 0xffffffffu;
        if (e < num_pairs) {
            const uint32_t id = global_ptr(point_list)[e];
            if (id < P) key = id;
        }
        global_ptr(keys)[e] = key;
        global_ptr(slots)[e] = e;
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
    // the Gaussian's run in the sorted keys
    uint32_t lo = 0u, hi = a.R;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (global_ptr(a.keys)[mid] < i)
            lo = mid + 1u;
        else
            hi = mid;
    }
    ImpScore view;
    imp_score_clear(view);
    uint32_t j = lo;
    for (; j < a.R && global_ptr(a.keys)[j] == i; j++) {
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
    const ImpScore o = imp_fold(view, imp_run_complete(j - lo, global_ptr(a.tiles)[i]), a.accumulate != 0, held);
    if (a.sum) global_ptr(a.sum)[i] = o.sum;
    if (a.max) global_ptr(a.max)[i] = o.max;
    if (a.count) global_ptr(a.count)[i] = o.count;
    if (a.views) global_ptr(a.views)[i] = o.views;
}

// the workspace: the rows, the (id, slot) arrays before and after the sort, rocPRIM's temp storage
struct ImpWork {
    ImpRow* rows;
    uint32_t *keys_in, *slots_in, *keys_out, *slots_out;
    char* temp;
    char* end;
    static ImpWork carve(char* base, size_t R, size_t temp_bytes)
    {
        Carver c(base);
        ImpWork w;
        w.rows = c.take<ImpRow>(R * kImpQuads);
        w.keys_in = c.take<uint32_t>(R);
        w.slots_in = c.take<uint32_t>(R);
        w.keys_out = c.take<uint32_t>(R);
        w.slots_out = c.take<uint32_t>(R);
        w.temp = c.take<char>(temp_bytes);
        w.end = c.p;
        return w;
    }
};

size_t sort_temp_bytes(size_t R)   // asked once per R: the query is host work, and a captured call must not repeat it
{
    static std::mutex mu;
    static std::map<size_t, size_t> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(R);
    if (it != known.end()) return it->second;
    size_t bytes = 0;
    R3_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     R, 0, 32, (hipStream_t)0));
    known[R] = bytes;
    return bytes;
}

void check_dims(const char* what, int P, int R, int width, int height)
{
    if (width < 1 || height < 1 || P < 0 || R < 0)
        throw Error(std::string(what) + ": need width, height >= 1 and P, R >= 0, got P = " + std::to_string(P) + ", R = " +
                    std::to_string(R) + ", " + std::to_string(width) + "x" + std::to_string(height));
}

}  // namespace

}  // namespace r3

extern "C" {

size_t r3dgs_contribution_scores_workspace_bytes(int P, int R, int width, int height)
{
    size_t out = 0;
    r3::guarded_call([&]() {
        using namespace r3;
        check_dims("contribution_scores_workspace_bytes", P, R, width, height);
        if (P == 0 || R == 0) return 0;
        out = (size_t)reinterpret_cast<uintptr_t>(ImpWork::carve(nullptr, (size_t)R, sort_temp_bytes((size_t)R)).end) + kAlign;
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
        check_dims("contribution_scores", P, R, width, height);
        if (accumulate != 0 && accumulate != 1)
            throw Error("contribution_scores: accumulate must be 0 or 1, got " + std::to_string(accumulate));
        const TileGrid grid = grid_of(width, height);
        const size_t N = (size_t)width * height, Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("contribution_scores: the image has too many tiles for one launch");
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
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("contribution_scores: state buffers must not be NULL");
        if (!workspace) throw Error("contribution_scores: the workspace must not be NULL");
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
        size_t temp = sort_temp_bytes((size_t)R);
        const ImpWork w = ImpWork::carve(workspace, (size_t)R, temp);

        ImpArgs a;
        a.ranges = st.img.ranges;
        a.point_list = st.bin.point_list;
        a.rec = st.geom.rec;
        a.n_contrib = st.img.n_contrib;
        a.quad_depth = st.img.quad_depth;
        a.weight = pixel_weight;
        a.W = width;
        a.H = height;
        a.gx = (int)grid.gx;
        a.nblocks = (uint32_t)(Tn * 4);
        a.P = (uint32_t)P;
        a.R = (uint32_t)R;
        a.rows = w.rows;
        a.T_check = T_check;
        a.n_check = n_check;
        hipLaunchKernelGGL(imp_walk_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("contribution scores, walk", s, false);
        if (!scores) return 0;

        const uint32_t key_blocks = (uint32_t)std::min<size_t>(((size_t)R + 255) / 256, 4096);
        hipLaunchKernelGGL(imp_keys_kernel, dim3(key_blocks), dim3(256), 0, s, st.geom.header, st.bin.point_list, (uint32_t)P,
                           (uint32_t)R, w.keys_in, w.slots_in);
        check_launch("contribution scores, keys", s, false);
        R3_HIP(rocprim::radix_sort_pairs(w.temp, temp, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)R, 0, 32, s));

        ImpSumArgs g;
        g.tiles = st.geom.tiles;
        g.keys = w.keys_out;
        g.slots = w.slots_out;
        g.rows = w.rows;
        g.P = (uint32_t)P;
        g.R = (uint32_t)R;
        g.accumulate = accumulate;
        g.sum = score_sum;
        g.max = score_max;
        g.count = score_count;
        g.views = score_views;
        hipLaunchKernelGGL(imp_gauss_kernel, dim3(((uint32_t)P + 255u) / 256u), dim3(256), 0, s, g);
        check_launch("contribution scores, per-Gaussian fold", s, false);
        return 0;
    });
}

}  // extern "C"
