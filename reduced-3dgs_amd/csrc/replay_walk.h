// replay_walk.h -- what the replay passes (aux_maps.hip, aux_bwd.hip, distortion.hip, feature_maps.hip, importance.hip) share
// up to "this chunk's mask is known and its records are in LDS": the lane geometry, the walk span, the staged record, the
// gather and the pre-test, and the two full-wave reductions.  The walk's contract is DESIGN.md "Replay passes"; the
// per-entry loops differ for real reasons (batched alphas, walk direction, the sums reduced) and stay in the kernels.
// The index arithmetic is R3_HD and checked on the CPU (tests/test_replay_walk_cpu.py); the rest is device code.
#pragma once
#include "blend_math.h"
#include "common.h"

namespace r3 {

constexpr int kWalkChunk = 64;   // list entries staged at a time: one per lane

// consecutive logical ids on one XCD, as the forward blend places its tiles (speed only); a permutation of [0, nblocks)
R3_HD uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

// One 64-lane wave per 8x8 quadrant of a tile (workgroup wg = tile * 4 + quadrant), one pixel per lane.
struct QuadLane {
    uint32_t tile;
    int quad;
    int px, py;
    float pxf, pyf;
    float qx0, qy0;   // the quadrant's first pixel
    bool inside;      // the pixel lies in the image
    size_t pix;       // its index there (only meaningful when inside)
};

R3_HD QuadLane quad_lane(uint32_t wg, int lane, int gx, int W, int H)
{
    QuadLane q;
    q.tile = wg >> 2;
    q.quad = (int)(wg & 3u);
    const int tile_x = (int)(q.tile % (uint32_t)gx), tile_y = (int)(q.tile / (uint32_t)gx);
    const int x0 = tile_x * kTile + (q.quad & 1) * 8, y0 = tile_y * kTile + (q.quad >> 1) * 8;
    q.qx0 = (float)x0;
    q.qy0 = (float)y0;
    q.px = x0 + (lane & 7);
    q.py = y0 + (lane >> 3);
    q.pxf = (float)q.px;
    q.pyf = (float)q.py;
    q.inside = q.px < W && q.py < H;
    q.pix = (size_t)W * (size_t)q.py + (size_t)q.px;
    return q;
}

// The part of a tile's list a quadrant walks: the list clamped into the blob of R pairs (an overflowed reservation cuts
// lists short; first + list_len <= R always), and of that the entries up to the quadrant's deepest contributor.
struct WalkSpan {
    uint32_t first;      // slot of the list's first entry
    uint32_t list_len;   // entries of the list inside the blob
    uint32_t len;        // entries walked: list positions [0, len), slots [first, first + len)
};

R3_HD WalkSpan walk_span(uint2 range, uint32_t quad_depth, uint32_t R)
{
    const uint32_t full = range.y > range.x ? range.y - range.x : 0u;
    WalkSpan s;
    s.first = range.x < R ? range.x : R;
    const uint32_t room = R - s.first;
    s.list_len = full < room ? full : room;
    s.len = s.list_len < quad_depth ? s.list_len : quad_depth;
    return s;
}

// the state a walk reads (DESIGN.md "Replay passes") and its launch geometry.  The seven pointers lead every kernel
// argument struct that derives from this: the first eight argument dwords are preloaded into SGPRs (build.py).
struct WalkArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const uint32_t* depth_key;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    int W, H, gx;
    uint32_t nblocks;   // 4 per tile
    uint32_t P, R;      // bounds of rec / depth_key and of point_list / the per-slot rows
};

inline WalkArgs walk_args_of(const PassStates& st, const TileGrid& grid, int P, int R, int width, int height)
{
    return {st.img.ranges, st.bin.point_list, st.geom.rec, st.geom.depth_key, st.img.final_T, st.img.n_contrib, st.img.quad_depth,
            width, height, (int)grid.gx, (uint32_t)(grid.n() * 4), (uint32_t)P, (uint32_t)R};
}

__device__ __forceinline__ WalkSpan load_walk_span(const WalkArgs& a, const QuadLane& q)
{
    return walk_span(global_ptr(a.ranges)[q.tile], global_ptr(a.quad_depth)[q.tile * 4u + (uint32_t)q.quad], a.R);
}

// 32 B: a staged list entry
struct WalkRec {
    float4 a;   // x, y, qa, qb
    float4 b;   // qc, op, two words of the unit's own (z, mapped depth, 1-based list position, dm/dz)
};

// the record of a gathered entry, the conic scaled as QSplat has it (blend_math.h scale_splat)
__device__ __forceinline__ WalkRec stage_rec(float4 nxa, float2 nxb, float bz, float bw)
{
    WalkRec r;
    r.a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
    r.b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, bz, bw);
    return r;
}

__device__ __forceinline__ QSplat load_splat(const WalkRec& r, float red)   // colour (red, 0, 0)
{
    QSplat s;
    s.x = r.a.x;
    s.y = r.a.y;
    s.qa = r.a.z;
    s.qb = r.a.w;
    s.qc = r.b.x;
    s.op = r.b.y;
    s.r = red;
    s.g = s.b = 0.f;
    return s;
}
__device__ __forceinline__ QSplat load_splat(const WalkRec& r) { return load_splat(r, 0.f); }
__device__ __forceinline__ QSplat load_splat_z(const WalkRec& r) { return load_splat(r, r.b.z); }   // b.z as the colour
__device__ __forceinline__ uint32_t load_pos1(const WalkRec& r) { return __float_as_uint(r.b.w); }   // b.w as a position

// The first 24 bytes of the GRec of list slot idx (pixel mean, conic, opacity), for idx < limit and an id inside the model;
// a kernel loads what else it stages (depth word, feature slice) inside its own `if (g.have)`.
struct WalkGather {
    float4 a;
    float2 b;
    uint32_t id;
    bool have;
};

__device__ __forceinline__ WalkGather gather_rec(const uint32_t* point_list, const GRec* rec, uint32_t P, uint32_t idx, uint32_t limit)
{
    WalkGather g;
    g.a = make_float4(0.f, 0.f, 0.f, 0.f);
    g.b = make_float2(0.f, 0.f);
    g.id = 0u;
    g.have = false;
    if (idx < limit) {
        g.id = global_ptr(point_list)[idx];
        if (g.id < P) {
            const auto* p = (const R3_GLOBAL float4*)global_ptr(rec + g.id);
            g.a = p[0];
            g.b = *(const R3_GLOBAL float2*)(p + 1);
            g.have = true;
        }
    }
    return g;
}

// the forward's region pre-test of a gathered entry against the quadrant, by the lane that holds the entry: the wave
// visits the entries the forward's wave visited
__device__ __forceinline__ bool walk_pretest(const float4& a, const float2& b, float qx0, float qy0)
{
    Splat mine;
    mine.x = a.x;
    mine.y = a.y;
    mine.cA = a.z;
    mine.cB = a.w;
    mine.cC = b.x;
    mine.op = b.y;
    mine.r = mine.g = mine.b = 0.f;
    return region_may_contribute(mine, qx0, qx0 + 7.f, qy0, qy0 + 7.f);
}

#define R3_WALK_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true))

// Full-wave reductions, the result in every lane, named for the order of their row steps: the two orders round differently
// and a caller keeps the one its reference sums in.
// row_ror: the backward blend's row steps (quad_perm, row_ror), then the two cross-row steps.
__device__ __forceinline__ float wave_sum_ror(float v)
{
    v += R3_WALK_DPP(v, 0xb1);    // quad_perm [1,0,3,2]
    v += R3_WALK_DPP(v, 0x4e);    // quad_perm [2,3,0,1]
    v += R3_WALK_DPP(v, 0x124);   // row_ror:4
    v += R3_WALK_DPP(v, 0x128);   // row_ror:8
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// mirror: the order of importance_math.h imp_tree_sum / imp_tree_max.  Every step is an exchange between two partners
// (lane ^ 1, lane ^ 2, the mirror of a half row, the mirror of a row -- after the first two steps a quad holds one value, so
// the mirrors pair quad with quad and half row with half row -- then lane ^ 16 and lane ^ 32), both of which combine the
// same two numbers.
__device__ __forceinline__ float wave_sum_mirror(float v)
{
    v += R3_WALK_DPP(v, 0xb1);    // quad_perm [1,0,3,2]
    v += R3_WALK_DPP(v, 0x4e);    // quad_perm [2,3,0,1]
    v += R3_WALK_DPP(v, 0x141);   // row_half_mirror
    v += R3_WALK_DPP(v, 0x140);   // row_mirror
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float wave_max_mirror(float v)
{
    v = fmaxf(v, R3_WALK_DPP(v, 0xb1));
    v = fmaxf(v, R3_WALK_DPP(v, 0x4e));
    v = fmaxf(v, R3_WALK_DPP(v, 0x141));
    v = fmaxf(v, R3_WALK_DPP(v, 0x140));
    v = fmaxf(v, __shfl_xor(v, 16));
    v = fmaxf(v, __shfl_xor(v, 32));
    return v;
}

}  // namespace r3
