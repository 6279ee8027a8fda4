// aux_bwd.hip -- gradients through the depth, alpha and median-depth maps (include/r3dgs_aux.h r3dgs_aux_maps_backward;
// the arithmetic is aux_math.h), gfx950.  A pass of its own behind any forward, like aux_maps.hip: it reads the three state
// blobs and writes only the caller's outputs and workspace.
//
// Four launches on the caller's stream, no host wait, no allocation, no atomics:
//   1. aux_bwd_pixel_kernel -- aux_maps_kernel's shape (one 64-lane wave per 8x8 quadrant of a tile, one pixel per lane,
//      the tile's list staged 64 entries at a time as 32-byte records in LDS, one chunk ahead of its use), walked back to
//      front from ImageState::quad_depth with T recovered from final_T by division, as the backward blend recovers it.  The
//      per-(pixel, entry) step is the backward blend's own (bwd_test / bwd_accumulate through aux_math.h) on a splat of
//      colour (z, 1, 0) and a pixel gradient (g_D, g_A, 0); build.py compiles this unit with blend.hip's flags.  Per entry
//      some lane blended, the wave reduces seven sums (2 for the pixel mean, 3 for the conic, 1 for the opacity, 1 for z)
//      and parks them in LDS; per chunk, lane j stores the 32-byte row of entry j -- the sums, or zeros for an entry no lane
//      of the quadrant blended -- at slab[(list slot * 4 + quadrant) * 8]; the slots of the list behind the quadrant's
//      deepest contributor get zero rows too.  Every (slot < num_pairs, quadrant) row is written in every call, by exactly
//      one wave: the slab needs no clearing and the reader no flags.
//   2. aux_bwd_keys_kernel -- (Gaussian id from point_list, list slot) per slot of the pair capacity; the key of a slot at or
//      beyond the header's num_pairs is 0xffffffff.
//   3. a stable rocPRIM radix sort of those pairs by id (temp storage from the caller's workspace).
//   4. aux_bwd_gauss_kernel -- one lane per Gaussian: its run of the sorted keys by binary search, its rows added in sorted
//      order (list slot ascending, quadrant 0..3) in double, then the per-Gaussian chain (aux_math.h aux_bwd_chain).  A
//      Gaussian that lost pairs to an overflowing reservation (its run is shorter than its tiles_touched) gets zero sums,
//      as the colour backward gives it zero 2D-stage gradients.
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "../../include/r3dgs_aux.h"
#include "aux_bwd_stage.h"
#include "aux_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kAuxChunk = 64;

struct AuxBwdArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const uint32_t* depth_key;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    const float* g_depth;    // [H*W] or nullptr (zero)
    const float* g_alpha;
    const float* g_median;
    int W, H, gx;
    uint32_t nblocks;
    uint32_t P, R;           // bounds of rec / depth_key and of point_list / the slab
    float* slab;             // [R][4][8]
};

struct AuxRec {   // 32 B: a staged list entry
    float4 a;     // x, y, qa, qb
    float4 b;     // qc, op, z, unused
};

__device__ __forceinline__ QSplat load_bwd_splat(const AuxRec& r)
{
    return aux_bwd_splat(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z);
}

__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

#define R3_AUX_DPP_ADD(v, ctrl) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))

// full-wave sum, the result in every lane: the backward blend's row steps (quad_perm, row_ror), then the two cross-row steps
__device__ __forceinline__ float wave_sum_all(float v)
{
    R3_AUX_DPP_ADD(v, 0xb1);    // quad_perm [1,0,3,2]
    R3_AUX_DPP_ADD(v, 0x4e);    // quad_perm [2,3,0,1]
    R3_AUX_DPP_ADD(v, 0x124);   // row_ror:4
    R3_AUX_DPP_ADD(v, 0x128);   // row_ror:8
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__global__ __launch_bounds__(64) void aux_bwd_pixel_kernel(const AuxBwdArgs a)
{
    __shared__ AuxRec s_rec[kAuxChunk];
    __shared__ float4 s_out[kAuxChunk][2];
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
    R3_GLOBAL float4* const rows = reinterpret_cast<R3_GLOBAL float4*>(global_ptr(a.slab));   // two float4 per row
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // the slots behind the walk: zero rows
    for (uint32_t k = len + (uint32_t)lane; k < list_len; k += kAuxChunk) {
        const size_t row = ((size_t)(first + k) * kAuxQuads + (size_t)quad) * 2;
        rows[row] = zero4;
        rows[row + 1] = zero4;
    }
    if (len == 0u) return;

    BwdPix p;
    float gM = 0.f;
    {
        float T = 1.f, gD = 0.f, gA = 0.f;
        uint32_t n = 0u;
        if (inside) {
            T = global_ptr(a.final_T)[pix];
            n = global_ptr(a.n_contrib)[pix];
            if (a.g_depth) gD = global_ptr(a.g_depth)[pix];
            if (a.g_alpha) gA = global_ptr(a.g_alpha)[pix];
            if (a.g_median) gM = global_ptr(a.g_median)[pix];
        }
        aux_bwd_pix_init(p, inside, T, n, gD, gA);
    }

    // software pipeline: the records of the next (shallower) chunk are gathered into registers while a chunk is walked
    float4 nxa = zero4;
    float2 nxb = make_float2(0.f, 0.f);
    uint32_t nxz = 0u;
    bool nxhave = false;
    auto gather = [&](uint32_t k) {   // k: position in the list; callers pass k < len only for the lanes that hold an entry
        nxhave = false;
        if (k < len) {
            const uint32_t id = global_ptr(a.point_list)[first + k];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                nxz = global_ptr(a.depth_key)[id];
                nxhave = true;
            }
        }
    };
    const uint32_t cfirst = ((len - 1u) / kAuxChunk) * kAuxChunk;
    gather(cfirst + (uint32_t)lane);
    SplatSums sg;
    aux_sums_clear(sg);
    for (uint32_t cbase = cfirst;; cbase -= kAuxChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, __uint_as_float(nxz), 0.f);
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
        if (cbase >= kAuxChunk) gather(cbase - kAuxChunk + (uint32_t)lane);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk some lane blended
        while (mask) {   // back to front: highest set bit first
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const QSplat s = load_bwd_splat(s_rec[j]);
            BwdEval e;
            const bool valid = bwd_test(s, pxf, pyf, cbase + (uint32_t)j, p, e);
            if (valid) aux_bwd_apply(s, e, p, gM, sg);
            if (__ballot(valid) != 0ull) {
                // the slab's order (aux_math.h aux_row_of): sx, sy, sxx, sxy, syy, sm, sz
                const float r0 = wave_sum_all(sg.sx), r1 = wave_sum_all(sg.sy), r2 = wave_sum_all(sg.sxx);
                const float r3 = wave_sum_all(sg.sxy), r4 = wave_sum_all(sg.syy), r5 = wave_sum_all(sg.sm);
                const float r6 = wave_sum_all(sg.r);
                if (lane == 0) {
                    s_out[j][0] = make_float4(r0, r1, r2, r3);
                    s_out[j][1] = make_float4(r4, r5, r6, 0.f);
                }
                contributed |= 1ull << j;
                aux_sums_clear(sg);
            }
        }
        __syncthreads();
        if (cbase + (uint32_t)lane < len) {
            const bool have = (contributed >> lane) & 1ull;
            const size_t row = ((size_t)(first + cbase + (uint32_t)lane) * kAuxQuads + (size_t)quad) * 2;
            float4 o0 = s_out[lane][0], o1 = s_out[lane][1];
            if (!have) o0 = o1 = make_float4(0.f, 0.f, 0.f, 0.f);
            rows[row] = o0;
            rows[row + 1] = o1;
        }
        if (cbase == 0u) break;
    }
}

// (Gaussian id, list slot) per slot of the pair capacity
__global__ __launch_bounds__(256) void aux_bwd_keys_kernel(const GeomHeader* hdr, const uint32_t* point_list, uint32_t P, uint32_t R,
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
    o.mean2D[0] = o.mean2D[1] = o.opacity = 0.f;
    for (int k = 0; k < 3; k++) o.mean3D[k] = o.scale[k] = 0.f;
    for (int k = 0; k < 4; k++) o.rot[k] = 0.f;
    for (int k = 0; k < 6; k++) o.cov6[k] = 0.f;
    if (global_ptr(a.radii)[i] > 0) {
        // the Gaussian's run in the sorted keys
        uint32_t lo = 0u, hi = a.R;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (global_ptr(a.keys)[mid] < i)
                lo = mid + 1u;
            else
                hi = mid;
        }
        double sums[kAuxSums];
        for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        uint32_t j = lo;
        for (; j < a.R && global_ptr(a.keys)[j] == i; j++) {
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
    if (a.dL_dmeans2D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dmeans2D) + 3 * (size_t)i;
        d[0] = o.mean2D[0];
        d[1] = o.mean2D[1];
        d[2] = 0.f;
    }
    if (a.dL_dmeans3D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dmeans3D) + 3 * (size_t)i;
        for (int k = 0; k < 3; k++) d[k] = o.mean3D[k];
    }
    if (a.dL_dopacity) global_ptr(a.dL_dopacity)[i] = o.opacity;
    if (a.dL_dscales) {
        R3_GLOBAL float* d = global_ptr(a.dL_dscales) + 3 * (size_t)i;
        for (int k = 0; k < 3; k++) d[k] = o.scale[k];
    }
    if (a.dL_drotations) {
        R3_GLOBAL float* d = global_ptr(a.dL_drotations) + 4 * (size_t)i;
        for (int k = 0; k < 4; k++) d[k] = o.rot[k];
    }
    if (a.dL_dcov3D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dcov3D) + 6 * (size_t)i;
        for (int k = 0; k < 6; k++) d[k] = o.cov6[k];
    }
}

// the workspace: the slab, the (id, slot) arrays before and after the sort, rocPRIM's temp storage
struct AuxBwdWork {
    float* slab;
    uint32_t *keys_in, *slots_in, *keys_out, *slots_out;
    char* temp;
    char* end;
    static AuxBwdWork carve(char* base, size_t R, size_t temp_bytes)
    {
        Carver c(base);
        AuxBwdWork w;
        w.slab = c.take<float>(R * kAuxQuads * kAuxRowFloats);
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

// ---- the second stage, shared with the units that write the same slab (aux_bwd_stage.h) ---------------------------------
size_t aux_bwd_workspace_bytes(size_t R)
{
    return (size_t)reinterpret_cast<uintptr_t>(AuxBwdWork::carve(nullptr, R, sort_temp_bytes(R)).end) + kAlign;
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
}

void aux_bwd_check_geom(const char* what, const AuxBwdGeom& g)
{
    if (!g.viewmatrix || !g.projmatrix || !g.means3D || !g.radii)
        throw Error(std::string(what) + ": viewmatrix, projmatrix, means3D and radii must not be NULL");
    if (!g.cov3D_precomp && (!g.scales || !g.rotations))
        throw Error(std::string(what) + ": need scales and rotations, or cov3D_precomp");
}

void aux_bwd_second_stage(const PassStates& st, int P, int R, int width, int height, const AuxBwdGeom& in, char* workspace,
                          hipStream_t s)
{
    size_t temp = sort_temp_bytes((size_t)R);
    const AuxBwdWork w = AuxBwdWork::carve(workspace, (size_t)R, temp);
    const uint32_t key_blocks = (uint32_t)std::min<size_t>(((size_t)R + 255) / 256, 4096);
    hipLaunchKernelGGL(aux_bwd_keys_kernel, dim3(key_blocks), dim3(256), 0, s, st.geom.header, st.bin.point_list, (uint32_t)P,
                       (uint32_t)R, w.keys_in, w.slots_in);
    check_launch("aux maps backward, keys", s, false);
    R3_HIP(rocprim::radix_sort_pairs(w.temp, temp, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)R, 0, 32, s));

    AuxGaussArgs g;
    g.rec = st.geom.rec;
    g.radii = in.radii;
    g.tiles = st.geom.tiles;
    g.keys = w.keys_out;
    g.slots = w.slots_out;
    g.slab = w.slab;
    g.view = in.viewmatrix;
    g.proj = in.projmatrix;
    g.means3D = in.means3D;
    g.scales = in.scales;
    g.rotations = in.rotations;
    g.cov3D_precomp = in.cov3D_precomp;
    g.tan_fovx = in.tan_fovx;
    g.tan_fovy = in.tan_fovy;
    g.scale_modifier = in.scale_modifier;
    g.W = width;
    g.H = height;
    g.P = (uint32_t)P;
    g.R = (uint32_t)R;
    g.dL_dmeans2D = in.dL_dmeans2D;
    g.dL_dmeans3D = in.dL_dmeans3D;
    g.dL_dopacity = in.dL_dopacity;
    g.dL_dscales = in.dL_dscales;
    g.dL_drotations = in.dL_drotations;
    g.dL_dcov3D = in.dL_dcov3D;
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
        check_dims("aux_maps_backward_workspace_bytes", P, R, width, height);
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
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_dims("aux_maps_backward", P, R, width, height);
        if (P == 0) return 0;   // every output has P rows
        const AuxBwdGeom geom = {viewmatrix, projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                 cov3D_precomp, radii, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D};
        const bool no_upstream = !dL_ddepth && !dL_dalpha && !dL_dmedian;
        if (R == 0 || no_upstream) {   // nothing to walk: zeros, the blobs are not read
            aux_bwd_zero_outputs(P, geom, s);
            return 0;
        }
        if (!geom.any_output()) return 0;
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("aux_maps_backward: state buffers must not be NULL");
        if (!workspace) throw Error("aux_maps_backward: the workspace must not be NULL");
        aux_bwd_check_geom("aux_maps_backward", geom);
        const TileGrid grid = grid_of(width, height);
        const size_t Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("aux_maps_backward: the image has too many tiles for one launch");
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);

        AuxBwdArgs a;
        a.ranges = st.img.ranges;
        a.point_list = st.bin.point_list;
        a.rec = st.geom.rec;
        a.depth_key = st.geom.depth_key;
        a.final_T = st.img.final_T;
        a.n_contrib = st.img.n_contrib;
        a.quad_depth = st.img.quad_depth;
        a.g_depth = dL_ddepth;
        a.g_alpha = dL_dalpha;
        a.g_median = dL_dmedian;
        a.W = width;
        a.H = height;
        a.gx = (int)grid.gx;
        a.nblocks = (uint32_t)(Tn * 4);
        a.P = (uint32_t)P;
        a.R = (uint32_t)R;
        a.slab = aux_bwd_slab(workspace, (size_t)R);
        hipLaunchKernelGGL(aux_bwd_pixel_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("aux maps backward, pixel pass", s, false);
        aux_bwd_second_stage(st, P, R, width, height, geom, workspace, s);
        return 0;
    });
}

}  // extern "C"
