// distortion.hip -- the depth-distortion map (the squared form of the 2DGS regulariser) and the pixel pass of the gradients
// through it, replayed from the state a forward pass left (include/r3dgs_distortion.h; the arithmetic is distortion_math.h),
// gfx950.  A pass of its own behind any forward, like aux_maps.hip / aux_bwd.hip: it reads the three state blobs and writes
// only the caller's outputs and workspace.
//
//   dist_map_kernel -- aux_maps_kernel's shape: one 64-lane wave per 8x8 quadrant of a tile, one pixel per lane, the tile's
//     list staged 64 entries at a time as 32-byte records in LDS one chunk ahead of its use, the forward's region pre-test by
//     the lane that holds the entry, the walk ended at the quadrant's deepest contributor.  The staging lane maps the entry's
//     view depth and shifts it by the mapped depth of the tile's first list entry (once per entry, not per pixel); the
//     per-(pixel, entry) step is the forward's own (fwd_alpha / fwd_apply through distortion_math.h), so the weights are the
//     forward's.  Writes distortion [H*W] and, when asked, the shifted moments S1, S2 [2, H*W].
//   dist_bwd_pixel_kernel -- aux_bwd_pixel_kernel's shape, walked back to front with T recovered from final_T by division;
//     the step is the backward blend's on a splat of colour c_k (three FMAs per lane from the broadcast mapped depth) under
//     the pixel gradient g.  It writes aux_bwd's 32-byte slab rows -- seven wave sums per (list slot, quadrant), zero rows for
//     entries nobody blended and for the slots behind the walk -- and aux_bwd.hip's second stage (aux_bwd_stage.h: keys,
//     stable sort, per-Gaussian double sums, chain) does the rest.
// No atomics, no host wait, no allocation, no scratch; the order of every sum is fixed by the data alone.  build.py compiles
// this unit with blend.hip's flags.
#include <string>

#include "../../include/r3dgs_distortion.h"
#include "aux_bwd_stage.h"
#include "common.h"
#include "distortion_math.h"

namespace r3 {

namespace {

constexpr int kDistChunk = 64;
constexpr int kDistBatch = 4;   // entries whose alphas are evaluated side by side before they are composited in order

struct DistRec {   // 32 B: a staged list entry
    float4 a;      // x, y, qa, qb
    float4 b;      // qc, op, shifted mapped depth, forward: 1-based list position (bits) / backward: dm/dz
};

struct DistArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const uint32_t* depth_key;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    int W, H, gx;
    uint32_t nblocks;
    uint32_t P, R;           // bounds of rec / depth_key and of point_list / the slab
    float near, far;
    float* distortion;       // forward outputs (either may be nullptr)
    float* moments;
    const float* g;          // backward inputs
    const float* saved;
    float* slab;             // backward output: [R][4][8]
};

__device__ __forceinline__ QSplat load_dist_splat(const DistRec& r)
{
    return aux_splat(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z);
}

// consecutive logical ids on one XCD, as the forward blend places its tiles (speed only)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

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
    __shared__ DistRec s_rec[kDistChunk];
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
    const size_t N = (size_t)a.W * (size_t)a.H;

    const uint2 range = global_ptr(a.ranges)[tile];
    // the walk: from the list's start to the deepest contributor of this quadrant, inside the list and inside the blob
    uint32_t len = range.y > range.x ? range.y - range.x : 0u;
    len = min(len, global_ptr(a.quad_depth)[tile * 4u + (uint32_t)quad]);
    const uint32_t first = min(range.x, a.R);
    const uint32_t end = first + min(len, a.R - first);
    const uint32_t n = inside ? global_ptr(a.n_contrib)[pix] : 0u;
    const DepthMap dm = tile_depth_map(a, range);
    DistPix p;
    dist_pix_init(p, inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float4 nxa = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 nxb = make_float2(0.f, 0.f);
    float nxm = 0.f;
    bool nxhave = false;
    auto gather = [&](uint32_t idx) {
        nxhave = false;
        if (idx < end) {
            const uint32_t id = global_ptr(a.point_list)[idx];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                nxm = mapped_depth_shifted(dm, __uint_as_float(global_ptr(a.depth_key)[id]));
                nxhave = true;
            }
        }
    };
    gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kDistChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, nxm, __uint_as_float(base - first + (uint32_t)lane + 1u));
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
        gather(base + kDistChunk + (uint32_t)lane);
        for (int left = __builtin_popcountll(mask); left >= kDistBatch; left -= kDistBatch) {
            QSplat sp[kDistBatch];
            uint32_t pos1[kDistBatch];
            float al[kDistBatch];
            bool inb[kDistBatch];
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                sp[i] = load_dist_splat(s_rec[j]);
                pos1[i] = __float_as_uint(s_rec[j].b.w);
            }
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) al[i] = fwd_alpha(sp[i], pxf, pyf, &inb[i]);
#pragma unroll
            for (int i = 0; i < kDistBatch; i++) dist_apply(sp[i], al[i], inb[i], pos1[i], n, p);
        }
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            dist_step(load_dist_splat(s_rec[j]), pxf, pyf, __float_as_uint(s_rec[j].b.w), n, p);
        }
    }
    if (inside) {
        if (a.distortion) global_ptr(a.distortion)[pix] = dist_value(p);
        if (a.moments) {
            global_ptr(a.moments)[pix] = dist_moment1(p);
            global_ptr(a.moments)[N + pix] = dist_moment2(p);
        }
    }
}

#define R3_DIST_DPP_ADD(v, ctrl) \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))

// full-wave sum, the result in every lane: aux_bwd.hip's (the backward blend's row steps, then the two cross-row steps)
__device__ __forceinline__ float wave_sum_all(float v)
{
    R3_DIST_DPP_ADD(v, 0xb1);    // quad_perm [1,0,3,2]
    R3_DIST_DPP_ADD(v, 0x4e);    // quad_perm [2,3,0,1]
    R3_DIST_DPP_ADD(v, 0x124);   // row_ror:4
    R3_DIST_DPP_ADD(v, 0x128);   // row_ror:8
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__global__ __launch_bounds__(64) void dist_bwd_pixel_kernel(const DistArgs a)
{
    __shared__ DistRec s_rec[kDistChunk];
    __shared__ float4 s_out[kDistChunk][2];
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
    const size_t N = (size_t)a.W * (size_t)a.H;

    const uint2 range = global_ptr(a.ranges)[tile];
    // the list inside the blob, and the part of it this quadrant walks: up to its deepest contributor
    const uint32_t full = range.y > range.x ? range.y - range.x : 0u;
    const uint32_t first = min(range.x, a.R);
    const uint32_t list_len = min(full, a.R - first);
    const uint32_t len = min(list_len, global_ptr(a.quad_depth)[tile * 4u + (uint32_t)quad]);
    R3_GLOBAL float4* const rows = reinterpret_cast<R3_GLOBAL float4*>(global_ptr(a.slab));   // two float4 per row
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // the slots behind the walk: zero rows
    for (uint32_t k = len + (uint32_t)lane; k < list_len; k += kDistChunk) {
        const size_t row = ((size_t)(first + k) * kAuxQuads + (size_t)quad) * 2;
        rows[row] = zero4;
        rows[row + 1] = zero4;
    }
    if (len == 0u) return;

    const DepthMap dm = tile_depth_map(a, range);
    BwdPix p;
    DistTotals tot;
    tot.A = tot.S1 = tot.S2 = 0.f;
    {
        float T = 1.f, g = 0.f;
        uint32_t n = 0u;
        if (inside) {
            T = global_ptr(a.final_T)[pix];
            n = global_ptr(a.n_contrib)[pix];
            g = global_ptr(a.g)[pix];
            tot.A = 1.0f - T;
            tot.S1 = global_ptr(a.saved)[pix];
            tot.S2 = global_ptr(a.saved)[N + pix];
        }
        dist_bwd_pix_init(p, inside, T, n, g);
    }

    // software pipeline: the records of the next (shallower) chunk are gathered into registers while a chunk is walked
    float4 nxa = zero4;
    float2 nxb = make_float2(0.f, 0.f);
    float nxm = 0.f, nxd = 0.f;
    bool nxhave = false;
    auto gather = [&](uint32_t k) {   // k: position in the list
        nxhave = false;
        if (k < len) {
            const uint32_t id = global_ptr(a.point_list)[first + k];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                const float z = __uint_as_float(global_ptr(a.depth_key)[id]);
                nxm = mapped_depth_shifted(dm, z);
                nxd = mapped_depth_dz(dm, z);
                nxhave = true;
            }
        }
    };
    const uint32_t cfirst = ((len - 1u) / kDistChunk) * kDistChunk;
    gather(cfirst + (uint32_t)lane);
    SplatSums sg;
    aux_sums_clear(sg);
    for (uint32_t cbase = cfirst;; cbase -= kDistChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, nxm, nxd);
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
        if (cbase >= kDistChunk) gather(cbase - kDistChunk + (uint32_t)lane);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk some lane blended
        while (mask) {   // back to front: highest set bit first
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const QSplat s = load_dist_splat(s_rec[j]);
            const float dmdz = s_rec[j].b.w;
            BwdEval e;
            const bool valid = bwd_test(s, pxf, pyf, cbase + (uint32_t)j, p, e);
            if (valid) dist_bwd_apply(s, dmdz, e, p, tot, sg);
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

void check_call(const char* what, int P, int R, int width, int height, float near, float far)
{
    if (width < 1 || height < 1 || P < 0 || R < 0)
        throw Error(std::string(what) + ": need width, height >= 1 and P, R >= 0, got P = " + std::to_string(P) + ", R = " +
                    std::to_string(R) + ", " + std::to_string(width) + "x" + std::to_string(height));
    if (!depth_map_valid(near, far))
        throw Error(std::string(what) + ": need near = far = 0 (the linear mapping) or 0 < near < far, got near = " +
                    std::to_string(near) + ", far = " + std::to_string(far));
}

DistArgs args_of(const PassStates& st, int P, int R, int width, int height, const TileGrid& grid, float near, float far)
{
    DistArgs a;
    a.ranges = st.img.ranges;
    a.point_list = st.bin.point_list;
    a.rec = st.geom.rec;
    a.depth_key = st.geom.depth_key;
    a.final_T = st.img.final_T;
    a.n_contrib = st.img.n_contrib;
    a.quad_depth = st.img.quad_depth;
    a.W = width;
    a.H = height;
    a.gx = (int)grid.gx;
    a.nblocks = (uint32_t)(grid.n() * 4);
    a.P = (uint32_t)P;
    a.R = (uint32_t)R;
    a.near = near;
    a.far = far;
    a.distortion = a.moments = a.slab = nullptr;
    a.g = a.saved = nullptr;
    return a;
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
        const TileGrid grid = grid_of(width, height);
        const size_t N = (size_t)width * height, Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("distortion_map: the image has too many tiles for one launch");
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            if (distortion) R3_HIP(hipMemsetAsync(distortion, 0, sizeof(float) * N, s));
            if (saved_moments) R3_HIP(hipMemsetAsync(saved_moments, 0, sizeof(float) * 2 * N, s));
            return 0;
        }
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("distortion_map: state buffers must not be NULL");
        if (!distortion && !saved_moments) return 0;
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
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
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_call("distortion_map_backward", P, R, width, height, near, far);
        if (P == 0) return 0;   // every output has P rows
        const AuxBwdGeom geom = {viewmatrix, projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                 cov3D_precomp, radii, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D};
        if (R == 0 || !dL_ddistortion) {   // nothing to walk: zeros, the blobs are not read
            aux_bwd_zero_outputs(P, geom, s);
            return 0;
        }
        if (!geom.any_output()) return 0;
        if (!geom_buffer || !binning_buffer || !image_buffer)
            throw Error("distortion_map_backward: state buffers must not be NULL");
        if (!saved_moments) throw Error("distortion_map_backward: saved_moments must not be NULL");
        if (!workspace) throw Error("distortion_map_backward: the workspace must not be NULL");
        aux_bwd_check_geom("distortion_map_backward", geom);
        const TileGrid grid = grid_of(width, height);
        if (grid.n() * 4 > 0x7fffffffull) throw Error("distortion_map_backward: the image has too many tiles for one launch");
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
        DistArgs a = args_of(st, P, R, width, height, grid, near, far);
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
