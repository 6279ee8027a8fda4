// aux_maps.hip -- expected depth, accumulated opacity and median depth per pixel, replayed from the state a forward pass
// left (include/r3dgs_aux.h; the arithmetic is aux_math.h), gfx950.
//
// A pass of its own behind any forward: it reads GeomState::rec (pixel mean, conic, opacity) and GeomState::depth_key (the
// float bits of the view depth), BinState::point_list, ImageState::ranges / n_contrib / final_T / quad_depth, and writes only
// the caller's output arrays -- the blobs stay as the forward left them, for the backward.
//
// Structure: the forward blend's (blend.hip) without the colour.
//   * one 64-lane wave per 8x8 quadrant of a tile, one pixel per lane, single-wave workgroups;
//   * the tile's list is fetched 64 entries at a time, one chunk ahead of its use: lane j gathers the first 32 bytes of the
//     GRec of entry j and its depth word, and parks them in LDS as a 32-byte record (x, y, scaled conic, opacity, z, list
//     position): two ds_write_b128 per lane, broadcast reads -- no bank conflicts either way; 2 KB of LDS per workgroup;
//   * the walk ends at the deepest contributor of the quadrant (ImageState::quad_depth, the maximum of n_contrib the forward
//     left), a pixel looks at no entry behind its own n_contrib;
//   * lane j runs the forward's region pre-test for entry j, so the wave visits the entries the forward's wave visited;
//   * the per-(pixel, entry) step is the forward's own (fwd_alpha / fwd_apply through aux_math.h), and build.py compiles this
//     unit with blend.hip's flags: T after every entry, the final T and the last contributor are the forward's bit for bit
//     (r3dgs_aux_maps hands them out as T_check / n_check and the tests hold them to final_T / n_contrib).
// Plain vector stores, no atomics.
#include <string>

#include "../../include/r3dgs_aux.h"
#include "aux_math.h"
#include "common.h"

namespace r3 {

namespace {

constexpr int kAuxChunk = 64;
constexpr int kAuxBatch = 4;   // entries whose alphas are evaluated side by side before they are composited in order

struct AuxArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const uint32_t* depth_key;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    int W, H, gx;
    uint32_t nblocks;
    uint32_t P, R;           // bounds of rec / depth_key and of point_list
    float* depth;
    float* alpha;
    float* median;
    float* T_check;
    uint32_t* n_check;
};

struct AuxRec {   // 32 B: a staged list entry
    float4 a;     // x, y, qa, qb
    float4 b;     // qc, op, z, 1-based list position (bits)
};

__device__ __forceinline__ QSplat load_aux_splat(const AuxRec& r)
{
    return aux_splat(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z);
}

__device__ __forceinline__ uint32_t staged_pos1(const AuxRec& r) { return __float_as_uint(r.b.w); }

// consecutive logical ids on one XCD, as the forward blend places its tiles (speed only)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

__global__ __launch_bounds__(64) void aux_maps_kernel(const AuxArgs a)
{
    __shared__ AuxRec s_rec[kAuxChunk];
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
    // the walk: from the list's start to the deepest contributor of this quadrant, inside the list and inside the blob
    uint32_t len = range.y > range.x ? range.y - range.x : 0u;
    len = min(len, global_ptr(a.quad_depth)[tile * 4u + (uint32_t)quad]);
    const uint32_t first = min(range.x, a.R);
    const uint32_t end = first + min(len, a.R - first);
    const uint32_t n = inside ? global_ptr(a.n_contrib)[pix] : 0u;
    AuxPix p;
    aux_pix_init(p, inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float4 nxa = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 nxb = make_float2(0.f, 0.f);
    uint32_t nxz = 0u;
    bool nxhave = false;
    auto gather = [&](uint32_t idx) {
        nxhave = false;
        if (idx < end) {
            const uint32_t id = global_ptr(a.point_list)[idx];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                nxz = global_ptr(a.depth_key)[id];
                nxhave = true;
            }
        }
    };
    gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kAuxChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, __uint_as_float(nxz),
                                    __uint_as_float(base - first + (uint32_t)lane + 1u));
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
        gather(base + kAuxChunk + (uint32_t)lane);
        for (int left = __builtin_popcountll(mask); left >= kAuxBatch; left -= kAuxBatch) {
            QSplat sp[kAuxBatch];
            uint32_t pos1[kAuxBatch];
            float al[kAuxBatch];
            bool inb[kAuxBatch];
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1ull;
                sp[i] = load_aux_splat(s_rec[j]);
                pos1[i] = staged_pos1(s_rec[j]);
            }
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) al[i] = fwd_alpha(sp[i], pxf, pyf, &inb[i]);
#pragma unroll
            for (int i = 0; i < kAuxBatch; i++) aux_apply(sp[i], al[i], inb[i], pos1[i], n, p);
        }
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            aux_step(load_aux_splat(s_rec[j]), pxf, pyf, staged_pos1(s_rec[j]), n, p);
        }
    }
    if (inside) {
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
        if (width < 1 || height < 1 || P < 0 || R < 0)
            throw Error("aux_maps: need width, height >= 1 and P, R >= 0, got P = " + std::to_string(P) + ", R = " +
                        std::to_string(R) + ", " + std::to_string(width) + "x" + std::to_string(height));
        const TileGrid grid = grid_of(width, height);
        const size_t N = (size_t)width * height, Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("aux_maps: the image has too many tiles for one launch");
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            float* const maps[4] = {depth, alpha, median_depth, T_check};
            for (float* m : maps)
                if (m) R3_HIP(hipMemsetAsync(m, 0, sizeof(float) * N, s));
            if (n_check) R3_HIP(hipMemsetAsync(n_check, 0, sizeof(uint32_t) * N, s));
            return 0;
        }
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("aux_maps: state buffers must not be NULL");
        if (!depth && !alpha && !median_depth && !T_check && !n_check) return 0;
        // (the arrays read here lie in front of the geometry blob's temp storage and of its optional tail: their offsets
        // are those of every forward's carve, lean or full)
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
        AuxArgs a;
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
        a.nblocks = (uint32_t)(Tn * 4);
        a.P = (uint32_t)P;
        a.R = (uint32_t)R;
        a.depth = depth;
        a.alpha = alpha;
        a.median = median_depth;
        a.T_check = T_check;
        a.n_check = n_check;
        hipLaunchKernelGGL(aux_maps_kernel, dim3(a.nblocks), dim3(64), 0, s, a);
        check_launch("aux maps", s, false);
        return 0;
    });
}

}  // extern "C"
