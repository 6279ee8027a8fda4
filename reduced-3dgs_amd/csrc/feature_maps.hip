// feature_maps.hip -- a per-Gaussian feature vector F[P, C] blended into a [C, H, W] map, and the gradients through it
// (include/r3dgs_features.h; the arithmetic is feature_math.h), gfx950.  Passes of their own behind any forward, like
// aux_maps.hip / aux_bwd.hip: they read the three state blobs and write only the caller's outputs and workspace.
//
// Channels go in register-resident groups of NC = 4, 8 or 16 (the smallest that holds C, 16 beyond); a map of more channels
// than a group is a further walk per group, over the second grid dimension.
//
// Forward, feat_fwd_kernel<NC> -- aux_maps_kernel's shape: one 64-lane wave per (8x8 quadrant of a tile, channel group), one
// pixel per lane; the tile's list is fetched 64 entries at a time, one chunk ahead of its use: lane j gathers the first 32
// bytes of the GRec of entry j and the group's slice of its feature row (16-byte loads when the rows allow it) and parks
// both in LDS -- a 32-byte record and NC floats beside it, 6 KB per workgroup at NC = 16; the walk ends at the quadrant's
// deepest contributor (ImageState::quad_depth), lane j runs the forward's region pre-test for entry j, and the step is the
// forward's own (feature_math.h feat_step).  Plain vector stores; a partial tile writes only the pixels inside the image.
//
// Backward, four or five launches on the caller's stream (the route of aux_bwd.hip; no host wait, no allocation, no atomics):
//   1. feat_bwd_pixel_kernel<NC, GEOM, FEAT> -- the same shape walked back to front with T recovered from final_T by
//      division.  Per entry some lane blended, the wave reduces the group's NC channel sums and (GEOM) the six geometric
//      sums with a TRANSPOSING reduction: at every step a lane hands half of its values to its partner and keeps the sums
//      of the other half, so N values cost N - 1 + (6 - log2 N) shuffles instead of 6 N, and lane l ends up with the
//      whole-wave sum of value feat_sum_slot(l).  Per chunk, lane j stores the rows of entry j -- the sums, or zeros for an
//      entry no lane blended -- at (list slot, quadrant[, group]); the slots behind the walk get zero rows.  Every row of
//      every slot < num_pairs is written in every call by exactly one wave: the slabs need no clearing.
//      The backward's recurrence is linear in the channels: each group carries its own and their geometric sums add up.
//   2. feat_keys_kernel, 3. a stable rocPRIM radix sort of (Gaussian id, list slot) by id.
//   4. feat_bwd_feature_kernel -- one lane per (Gaussian, four channels): its run of the sorted keys by binary search, its
//      rows added in sorted order (slot ascending, quadrant 0..3) in double -> dL_dfeatures.
//   5. feat_bwd_gauss_kernel<F64> (GEOM) -- one lane per Gaussian: the six sums over (slot, quadrant, group) in double, then
//      aux_math.h aux_bwd_chain with a zero z sum.
// A Gaussian that lost pairs to an overflowed reservation (its run is shorter than its tiles_touched) gets zero rows.
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
// Workspace per pair, G = ceil(C / 16) groups (NC = 16): 4 x G x 64 B feature rows + 4 x G x 32 B geometric rows + 16 B of
// keys and slots = 384 G + 16 bytes, plus rocPRIM's temp storage.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "../../include/r3dgs_features.h"
#include "feature_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kChunk = 64;
constexpr int kGeoRow = 8;   // floats per geometric row: sx, sy, sxx, sxy, syy, sm, 0, 0

struct FeatRec {   // 32 B: a staged list entry
    float4 a;      // x, y, qa, qb
    float4 b;      // qc, op, unused, 1-based list position (bits; forward only)
};

__device__ __forceinline__ QSplat load_splat(const FeatRec& r) { return feat_splat(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y); }

// consecutive logical ids on one XCD, as the forward blend places its tiles (speed only)
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nblocks)
{
    const uint32_t per = nblocks >> 3;
    if (b >= per * 8) return b;
    return (b & 7u) * per + (b >> 3);
}

struct FeatArgs {
    const uint2* ranges;
    const uint32_t* point_list;
    const GRec* rec;
    const float* final_T;
    const uint32_t* n_contrib;
    const uint32_t* quad_depth;
    const float* features;   // [P, C]
    const float* g_out;      // backward: dL_dout [C, H*W]
    int W, H, gx, C;
    int vec4;                // the feature rows can be read as float4 (C % 4 == 0 and a 16-byte aligned base)
    uint32_t nblocks, ngroups;
    uint32_t P, R;           // bounds of rec / features and of point_list / the slabs
    float* out;              // forward: [C, H*W]
    float* slab_f;           // backward: [R][4][ngroups * NC]
    float* slab_g;           // backward: [R][4][ngroups][8]
};

// the group's slice of feature row `id`: channels c0 .. c0 + NC - 1, zero past C
template <int NC>
__device__ __forceinline__ void load_slice(const FeatArgs& a, uint32_t id, int c0, float (&f)[NC])
{
    const R3_GLOBAL float* row = global_ptr(a.features) + (size_t)id * (size_t)a.C + (size_t)c0;
    if (a.vec4) {
#pragma unroll
        for (int q = 0; q < NC / 4; q++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + 4 * q < a.C) v = *reinterpret_cast<const R3_GLOBAL float4*>(row + 4 * q);
            f[4 * q] = v.x;
            f[4 * q + 1] = v.y;
            f[4 * q + 2] = v.z;
            f[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < NC; c++) f[c] = c0 + c < a.C ? row[c] : 0.f;
    }
}

template <int NC>
__device__ __forceinline__ void park_slice(float4 (*s_feat)[kChunk], int lane, const float (&f)[NC])
{
#pragma unroll
    for (int q = 0; q < NC / 4; q++) s_feat[q][lane] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
}

template <int NC>
__device__ __forceinline__ void read_slice(const float4 (*s_feat)[kChunk], int j, float (&f)[NC])
{
#pragma unroll
    for (int q = 0; q < NC / 4; q++) {
        const float4 v = s_feat[q][j];
        f[4 * q] = v.x;
        f[4 * q + 1] = v.y;
        f[4 * q + 2] = v.z;
        f[4 * q + 3] = v.w;
    }
}

__device__ __forceinline__ bool pretest(const float4& a, const float2& b, float qx0, float qy0)
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

template <int NC>
__global__ __launch_bounds__(64) void feat_fwd_kernel(const FeatArgs a)
{
    __shared__ FeatRec s_rec[kChunk];
    __shared__ float4 s_feat[NC / 4][kChunk];
    const int lane = threadIdx.x;
    const uint32_t wg = xcd_remap(blockIdx.x, a.nblocks);
    const int c0 = (int)blockIdx.y * NC;
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
    FeatPix<NC> p;
    feat_pix_init<NC>(p, inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float4 nxa = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 nxb = make_float2(0.f, 0.f);
    float nxf[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) nxf[c] = 0.f;
    bool nxhave = false;
    auto gather = [&](uint32_t idx) {
        nxhave = false;
        if (idx < end) {
            const uint32_t id = global_ptr(a.point_list)[idx];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                load_slice<NC>(a, id, c0, nxf);
                nxhave = true;
            }
        }
    };
    gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, 0.f, __uint_as_float(base - first + (uint32_t)lane + 1u));
        park_slice<NC>(s_feat, lane, nxf);
        unsigned long long mask = __ballot(nxhave && pretest(nxa, nxb, qx0, qy0));
        __syncthreads();
        gather(base + kChunk + (uint32_t)lane);
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            float f[NC];
            read_slice<NC>(s_feat, j, f);
            feat_step<NC>(load_splat(s_rec[j]), pxf, pyf, __float_as_uint(s_rec[j].b.w), n, f, p);
        }
    }
    if (inside) {
        const size_t N = (size_t)a.W * (size_t)a.H;
#pragma unroll
        for (int c = 0; c < NC; c++)
            if (c0 + c < a.C) global_ptr(a.out)[(size_t)(c0 + c) * N + pix] = p.acc[c];
    }
}

// Whole-wave sums of N values per lane, N = 4, 8 or 16, in N - 1 + (6 - log2 N) shuffles: at step b a lane keeps the
// half of its values its bit b selects, added to its partner's copy of that half.  Returns, in lane l, the sum over all 64
// lanes of value feat_sum_slot<N>(l) (every value in N lanes' worth of copies; lanes 0 .. N - 1 hold them all).  Both partners
// add the same two numbers: the result does not depend on the lane that formed it.
template <int N>
__device__ __forceinline__ float wave_transpose_sum(float (&v)[N], int lane)
{
    constexpr int kSteps = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : -1;
    static_assert(kSteps > 0, "N: 4, 8 or 16");
#pragma unroll
    for (int b = 0; b < kSteps; b++) {
        const int half = N >> (b + 1);
        const bool up = (lane >> b) & 1;
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            if (i >= half) break;
            const float lo = v[i], hi = v[i + half];   // (values, not lvalues: a select of addresses would put v in scratch)
            float send = hi, keep = lo;
            if (up) {
                send = lo;
                keep = hi;
            }
            v[i] = keep + __shfl_xor(send, 1 << b);
        }
    }
    float r = v[0];
#pragma unroll
    for (int s = N; s < 64; s <<= 1) r += __shfl_xor(r, s);
    return r;
}

template <int N>
__device__ __forceinline__ int feat_sum_slot(int lane)   // which of the N values lane `lane` holds after wave_transpose_sum
{
    int idx = 0, b = 0;
    for (int half = N / 2; half >= 1; half >>= 1, b++) idx += ((lane >> b) & 1) * half;
    return idx;
}

template <int NC, bool GEOM, bool FEAT>
__global__ __launch_bounds__(64) void feat_bwd_pixel_kernel(const FeatArgs a)
{
    __shared__ FeatRec s_rec[kChunk];
    __shared__ float4 s_feat[GEOM ? NC / 4 : 1][kChunk];
    __shared__ float s_outf[FEAT ? kChunk : 1][NC];
    __shared__ float s_outg[GEOM ? kChunk : 1][kGeoRow];
    const int lane = threadIdx.x;
    const uint32_t wg = xcd_remap(blockIdx.x, a.nblocks);
    const uint32_t grp = blockIdx.y;
    const int c0 = (int)grp * NC;
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
    const size_t cpad = (size_t)a.ngroups * NC;
    R3_GLOBAL float* const slab_f = global_ptr(a.slab_f);
    R3_GLOBAL float* const slab_g = global_ptr(a.slab_g);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto frow = [&](uint32_t k) {   // the group's part of the feature row of list position k
        return reinterpret_cast<R3_GLOBAL float4*>(slab_f + ((size_t)(first + k) * 4 + (size_t)quad) * cpad + (size_t)c0);
    };
    auto grow = [&](uint32_t k) {
        return reinterpret_cast<R3_GLOBAL float4*>(slab_g + (((size_t)(first + k) * 4 + (size_t)quad) * a.ngroups + grp) * kGeoRow);
    };
    // the slots behind the walk: zero rows
    for (uint32_t k = len + (uint32_t)lane; k < list_len; k += kChunk) {
        if (FEAT) {
            R3_GLOBAL float4* r = frow(k);
#pragma unroll
            for (int q = 0; q < NC / 4; q++) r[q] = zero4;
        }
        if (GEOM) {
            R3_GLOBAL float4* r = grow(k);
            r[0] = zero4;
            r[1] = zero4;
        }
    }
    if (len == 0u) return;

    FeatBwdPix<NC> p;
    {
        float T = 1.f, g[NC];
        uint32_t n = 0u;
#pragma unroll
        for (int c = 0; c < NC; c++) g[c] = 0.f;
        if (inside) {
            T = global_ptr(a.final_T)[pix];
            n = global_ptr(a.n_contrib)[pix];
            const size_t N = (size_t)a.W * (size_t)a.H;
#pragma unroll
            for (int c = 0; c < NC; c++)
                if (c0 + c < a.C) g[c] = global_ptr(a.g_out)[(size_t)(c0 + c) * N + pix];
        }
        feat_bwd_pix_init<NC>(p, inside, T, n, g);
    }

    // software pipeline: the records of the next (shallower) chunk are gathered into registers while a chunk is walked
    float4 nxa = zero4;
    float2 nxb = make_float2(0.f, 0.f);
    float nxf[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) nxf[c] = 0.f;
    bool nxhave = false;
    auto gather = [&](uint32_t k) {   // k: position in the list
        nxhave = false;
        if (k < len) {
            const uint32_t id = global_ptr(a.point_list)[first + k];
            if (id < a.P) {
                const auto* g = (const R3_GLOBAL float4*)global_ptr(a.rec + id);
                nxa = g[0];
                nxb = *(const R3_GLOBAL float2*)(g + 1);
                if (GEOM) load_slice<NC>(a, id, c0, nxf);
                nxhave = true;
            }
        }
    };
    const uint32_t cfirst = ((len - 1u) / kChunk) * kChunk;
    gather(cfirst + (uint32_t)lane);
    FeatSums<NC> sg;
    feat_sums_clear<NC>(sg);
    const int fslot = feat_sum_slot<NC>(lane), gslot = feat_sum_slot<kGeoRow>(lane);
    for (uint32_t cbase = cfirst;; cbase -= kChunk) {
        __syncthreads();
        s_rec[lane].a = make_float4(nxa.x, nxa.y, (-0.5f * kLog2e) * nxa.z, -kLog2e * nxa.w);
        s_rec[lane].b = make_float4((-0.5f * kLog2e) * nxb.x, nxb.y, 0.f, 0.f);
        if (GEOM) park_slice<NC>(s_feat, lane, nxf);
        unsigned long long mask = __ballot(nxhave && pretest(nxa, nxb, qx0, qy0));
        __syncthreads();
        if (cbase >= kChunk) gather(cbase - kChunk + (uint32_t)lane);
        unsigned long long contributed = 0ull;   // wave-uniform: entries of this chunk some lane blended
        while (mask) {   // back to front: highest set bit first
            const int j = 63 - __builtin_clzll(mask);
            mask &= ~(1ull << j);
            const QSplat s = load_splat(s_rec[j]);
            float f[NC];
            if (GEOM) {
                read_slice<NC>(s_feat, j, f);
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++) f[c] = 0.f;
            }
            const bool valid = feat_bwd_step<NC, GEOM>(s, pxf, pyf, cbase + (uint32_t)j, f, p, sg);
            if (__ballot(valid) != 0ull) {
                if (FEAT) {
                    const float r = wave_transpose_sum<NC>(sg.f, lane);
                    if (lane < NC) s_outf[j][fslot] = r;
                }
                if (GEOM) {
                    float v[kGeoRow] = {sg.s.sx, sg.s.sy, sg.s.sxx, sg.s.sxy, sg.s.syy, sg.s.sm, 0.f, 0.f};
                    const float r = wave_transpose_sum<kGeoRow>(v, lane);
                    if (lane < kGeoRow) s_outg[j][gslot] = r;
                }
                contributed |= 1ull << j;
                feat_sums_clear<NC>(sg);
            }
        }
        __syncthreads();
        if (cbase + (uint32_t)lane < len) {
            const bool have = (contributed >> lane) & 1ull;
            if (FEAT) {
                R3_GLOBAL float4* r = frow(cbase + (uint32_t)lane);
#pragma unroll
                for (int q = 0; q < NC / 4; q++) {
                    float4 o = zero4;   // (assigned, not selected: a select of two lvalues is a select of addresses)
                    if (have) o = make_float4(s_outf[lane][4 * q], s_outf[lane][4 * q + 1], s_outf[lane][4 * q + 2], s_outf[lane][4 * q + 3]);
                    r[q] = o;
                }
            }
            if (GEOM) {
                R3_GLOBAL float4* r = grow(cbase + (uint32_t)lane);
                float4 o0 = zero4, o1 = zero4;
                if (have) {
                    o0 = make_float4(s_outg[lane][0], s_outg[lane][1], s_outg[lane][2], s_outg[lane][3]);
                    o1 = make_float4(s_outg[lane][4], s_outg[lane][5], 0.f, 0.f);
                }
                r[0] = o0;
                r[1] = o1;
            }
        }
        if (cbase == 0u) break;
    }
}

// (Gaussian id, list slot) per slot of the pair capacity
__global__ __launch_bounds__(256) void feat_keys_kernel(const GeomHeader* hdr, const uint32_t* point_list, uint32_t P, uint32_t R,
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

// the run of Gaussian i in the sorted keys: [lo, lo + count)
__device__ __forceinline__ uint32_t run_of(const uint32_t* keys, uint32_t R, uint32_t i, uint32_t* count)
{
    uint32_t lo = 0u, hi = R;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (global_ptr(keys)[mid] < i)
            lo = mid + 1u;
        else
            hi = mid;
    }
    uint32_t j = lo;
    while (j < R && global_ptr(keys)[j] == i) j++;
    *count = j - lo;
    return lo;
}

struct FeatSumArgs {
    const int* radii;
    const uint32_t* tiles;   // [P] tiles_touched: the pairs the forward wanted for the Gaussian
    const uint32_t* keys;    // [R] sorted ids
    const uint32_t* slots;   // [R] their list slots
    const float* slab_f;
    uint32_t P, R, cq;       // cq: float4 columns of a feature row (cpad / 4)
    int C;
    float* dL_dfeatures;
};

__global__ __launch_bounds__(256) void feat_bwd_feature_kernel(const FeatSumArgs a)
{
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)a.P * a.cq) return;
    const uint32_t i = (uint32_t)(t / a.cq), q = (uint32_t)(t % a.cq);
    if (4u * q >= (uint32_t)a.C) return;   // a column of padding only
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (global_ptr(a.radii)[i] > 0) {
        uint32_t count;
        const uint32_t lo = run_of(a.keys, a.R, i, &count);
        // a Gaussian whose pairs did not all fit the pass's reservation gets zeros instead of a partial sum
        if (count == global_ptr(a.tiles)[i]) {
            for (uint32_t j = lo; j < lo + count; j++) {
                const uint32_t slot = global_ptr(a.slots)[j];
                if (slot >= a.R) continue;
                const auto* rows = reinterpret_cast<const R3_GLOBAL float4*>(global_ptr(a.slab_f)) + (size_t)slot * 4 * a.cq + q;
#pragma unroll
                for (int qd = 0; qd < 4; qd++) {
                    const float4 r = rows[(size_t)qd * a.cq];
                    s0 += (double)r.x;
                    s1 += (double)r.y;
                    s2 += (double)r.z;
                    s3 += (double)r.w;
                }
            }
        }
    }
    R3_GLOBAL float* d = global_ptr(a.dL_dfeatures) + (size_t)i * (size_t)a.C + 4u * q;
    const double s[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if ((int)(4u * q) + k < a.C) d[k] = (float)s[k];
}

struct FeatGaussArgs {
    const GRec* rec;
    const int* radii;
    const uint32_t* tiles;
    const uint32_t* keys;
    const uint32_t* slots;
    const float* slab_g;
    const float *view, *proj;
    const float *means3D, *scales, *rotations, *cov3D_precomp;
    float tan_fovx, tan_fovy, scale_modifier;
    int W, H;
    uint32_t P, R, ngroups;
    float *dL_dmeans2D, *dL_dmeans3D, *dL_dopacity, *dL_dscales, *dL_drotations, *dL_dcov3D;
};

template <bool F64>
__global__ __launch_bounds__(64) void feat_bwd_gauss_kernel(const FeatGaussArgs a)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= a.P) return;
    AuxGaussGrad o;
    o.mean2D[0] = o.mean2D[1] = o.opacity = 0.f;
    for (int k = 0; k < 3; k++) o.mean3D[k] = o.scale[k] = 0.f;
    for (int k = 0; k < 4; k++) o.rot[k] = 0.f;
    for (int k = 0; k < 6; k++) o.cov6[k] = 0.f;
    if (global_ptr(a.radii)[i] > 0) {
        uint32_t count;
        const uint32_t lo = run_of(a.keys, a.R, i, &count);
        double sums[kAuxSums];
        for (int k = 0; k < kAuxSums; k++) sums[k] = 0.0;
        const uint32_t rows_per_slot = 4u * a.ngroups;
        for (uint32_t j = lo; j < lo + count; j++) {
            const uint32_t slot = global_ptr(a.slots)[j];
            if (slot >= a.R) continue;
            const auto* rows = reinterpret_cast<const R3_GLOBAL float4*>(global_ptr(a.slab_g)) + (size_t)slot * rows_per_slot * 2;
            for (uint32_t q = 0; q < rows_per_slot; q++) {   // quadrant 0..3, its groups in order
                const float4 r0 = rows[2 * q], r1 = rows[2 * q + 1];
                sums[0] += (double)r0.x;
                sums[1] += (double)r0.y;
                sums[2] += (double)r0.z;
                sums[3] += (double)r0.w;
                sums[4] += (double)r1.x;
                sums[5] += (double)r1.y;
            }
        }
        // a Gaussian whose pairs did not all fit the pass's reservation gets zero 2D-stage gradients instead of a partial sum
        if (count != global_ptr(a.tiles)[i])
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

int group_width(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : kFeatGroup; }

// the workspace: the two slabs, the (id, slot) arrays before and after the sort, rocPRIM's temp storage
struct FeatWork {
    float *slab_f, *slab_g;
    uint32_t *keys_in, *slots_in, *keys_out, *slots_out;
    char* temp;
    char* end;
    static FeatWork carve(char* base, size_t R, int C, size_t temp_bytes)
    {
        const size_t nc = (size_t)group_width(C), groups = ((size_t)C + nc - 1) / nc;
        Carver c(base);
        FeatWork w;
        w.slab_f = c.take<float>(R * 4 * groups * nc);
        w.slab_g = c.take<float>(R * 4 * groups * kGeoRow);
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

void check_dims(const char* what, int P, int R, int C, int width, int height)
{
    if (width < 1 || height < 1 || P < 0 || R < 0)
        throw Error(std::string(what) + ": need width, height >= 1 and P, R >= 0, got P = " + std::to_string(P) + ", R = " +
                    std::to_string(R) + ", " + std::to_string(width) + "x" + std::to_string(height));
    if (C < 1 || C > R3DGS_FEATURE_MAX_CHANNELS)
        throw Error(std::string(what) + ": need 1 <= C <= " + std::to_string(R3DGS_FEATURE_MAX_CHANNELS) + " channels, got C = " +
                    std::to_string(C));
}

FeatArgs base_args(const PassStates& st, const TileGrid& grid, int P, int R, int width, int height, const float* features, int C)
{
    FeatArgs a;
    std::memset(&a, 0, sizeof(a));
    a.ranges = st.img.ranges;
    a.point_list = st.bin.point_list;
    a.rec = st.geom.rec;
    a.final_T = st.img.final_T;
    a.n_contrib = st.img.n_contrib;
    a.quad_depth = st.img.quad_depth;
    a.features = features;
    a.W = width;
    a.H = height;
    a.gx = (int)grid.gx;
    a.C = C;
    a.vec4 = (C % 4 == 0) && (reinterpret_cast<uintptr_t>(features) % 16 == 0);
    a.nblocks = (uint32_t)(grid.n() * 4);
    const int nc = group_width(C);
    a.ngroups = (uint32_t)((C + nc - 1) / nc);
    a.P = (uint32_t)P;
    a.R = (uint32_t)R;
    return a;
}

template <bool GEOM, bool FEAT>
void launch_pixel(int nc, const FeatArgs& a, hipStream_t s)
{
    const dim3 grid(a.nblocks, a.ngroups);
    if (nc == 4)
        hipLaunchKernelGGL((feat_bwd_pixel_kernel<4, GEOM, FEAT>), grid, dim3(64), 0, s, a);
    else if (nc == 8)
        hipLaunchKernelGGL((feat_bwd_pixel_kernel<8, GEOM, FEAT>), grid, dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((feat_bwd_pixel_kernel<16, GEOM, FEAT>), grid, dim3(64), 0, s, a);
}

}  // namespace

}  // namespace r3

extern "C" {

int r3dgs_feature_maps(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                       const float* features, int C, float* out, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_dims("feature_maps", P, R, C, width, height);
        const TileGrid grid = grid_of(width, height);
        const size_t N = (size_t)width * height, Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("feature_maps: the image has too many tiles for one launch");
        if (!out) return 0;
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            R3_HIP(hipMemsetAsync(out, 0, sizeof(float) * N * (size_t)C, s));
            return 0;
        }
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("feature_maps: state buffers must not be NULL");
        if (!features) throw Error("feature_maps: features must not be NULL");
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
        FeatArgs a = base_args(st, grid, P, R, width, height, features, C);
        a.out = out;
        const dim3 g(a.nblocks, a.ngroups);
        const int nc = group_width(C);
        if (nc == 4)
            hipLaunchKernelGGL(feat_fwd_kernel<4>, g, dim3(64), 0, s, a);
        else if (nc == 8)
            hipLaunchKernelGGL(feat_fwd_kernel<8>, g, dim3(64), 0, s, a);
        else
            hipLaunchKernelGGL(feat_fwd_kernel<16>, g, dim3(64), 0, s, a);
        check_launch("feature maps", s, false);
        return 0;
    });
}

size_t r3dgs_feature_maps_backward_workspace_bytes(int P, int R, int C, int width, int height)
{
    size_t out = 0;
    r3::guarded_call([&]() {
        using namespace r3;
        check_dims("feature_maps_backward_workspace_bytes", P, R, C, width, height);
        if (P == 0 || R == 0) return 0;
        out = (size_t)reinterpret_cast<uintptr_t>(FeatWork::carve(nullptr, (size_t)R, C, sort_temp_bytes((size_t)R)).end) + kAlign;
        return 0;
    });
    return out;
}

int r3dgs_feature_maps_backward(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy,
                                const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                                const float* cov3D_precomp, const int* radii, const float* features, int C, const float* dL_dout,
                                float* dL_dfeatures, float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity,
                                float* dL_dscales, float* dL_drotations, float* dL_dcov3D, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_dims("feature_maps_backward", P, R, C, width, height);
        if (P == 0) return 0;   // every output has P rows
        const bool geom = dL_dmeans2D || dL_dmeans3D || dL_dopacity || dL_dscales || dL_drotations || dL_dcov3D;
        const bool feat = dL_dfeatures != nullptr;
        if (R == 0 || !dL_dout) {   // nothing to walk: zeros, the blobs are not read
            const size_t n = (size_t)P;
            if (dL_dfeatures) R3_HIP(hipMemsetAsync(dL_dfeatures, 0, sizeof(float) * (size_t)C * n, s));
            if (dL_dmeans2D) R3_HIP(hipMemsetAsync(dL_dmeans2D, 0, sizeof(float) * 3 * n, s));
            if (dL_dmeans3D) R3_HIP(hipMemsetAsync(dL_dmeans3D, 0, sizeof(float) * 3 * n, s));
            if (dL_dopacity) R3_HIP(hipMemsetAsync(dL_dopacity, 0, sizeof(float) * n, s));
            if (dL_dscales) R3_HIP(hipMemsetAsync(dL_dscales, 0, sizeof(float) * 3 * n, s));
            if (dL_drotations) R3_HIP(hipMemsetAsync(dL_drotations, 0, sizeof(float) * 4 * n, s));
            if (dL_dcov3D) R3_HIP(hipMemsetAsync(dL_dcov3D, 0, sizeof(float) * 6 * n, s));
            return 0;
        }
        if (!geom && !feat) return 0;
        if (!geom_buffer || !binning_buffer || !image_buffer) throw Error("feature_maps_backward: state buffers must not be NULL");
        if (!workspace) throw Error("feature_maps_backward: the workspace must not be NULL");
        if (!radii) throw Error("feature_maps_backward: radii must not be NULL");
        if (geom) {
            if (!features) throw Error("feature_maps_backward: the geometry gradients need features");
            if (!viewmatrix || !projmatrix || !means3D)
                throw Error("feature_maps_backward: the geometry gradients need viewmatrix, projmatrix and means3D");
            if (!cov3D_precomp && (!scales || !rotations))
                throw Error("feature_maps_backward: need scales and rotations, or cov3D_precomp");
        }
        const TileGrid grid = grid_of(width, height);
        const size_t Tn = grid.n();
        if (Tn * 4 > 0x7fffffffull) throw Error("feature_maps_backward: the image has too many tiles for one launch");
        const PassStates st = carve_pass(P, (uint32_t)R, width, height, {geom_buffer, binning_buffer, image_buffer}, 0);
        size_t temp = sort_temp_bytes((size_t)R);
        const FeatWork w = FeatWork::carve(workspace, (size_t)R, C, temp);

        FeatArgs a = base_args(st, grid, P, R, width, height, features, C);
        a.g_out = dL_dout;
        a.slab_f = w.slab_f;
        a.slab_g = w.slab_g;
        const int nc = group_width(C);
        if (geom && feat)
            launch_pixel<true, true>(nc, a, s);
        else if (geom)
            launch_pixel<true, false>(nc, a, s);
        else
            launch_pixel<false, true>(nc, a, s);
        check_launch("feature maps backward, pixel pass", s, false);

        const uint32_t key_blocks = (uint32_t)std::min<size_t>(((size_t)R + 255) / 256, 4096);
        hipLaunchKernelGGL(feat_keys_kernel, dim3(key_blocks), dim3(256), 0, s, st.geom.header, st.bin.point_list, (uint32_t)P,
                           (uint32_t)R, w.keys_in, w.slots_in);
        check_launch("feature maps backward, keys", s, false);
        R3_HIP(rocprim::radix_sort_pairs(w.temp, temp, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)R, 0, 32, s));

        if (feat) {
            FeatSumArgs f;
            f.radii = radii;
            f.tiles = st.geom.tiles;
            f.keys = w.keys_out;
            f.slots = w.slots_out;
            f.slab_f = w.slab_f;
            f.P = (uint32_t)P;
            f.R = (uint32_t)R;
            f.cq = a.ngroups * (uint32_t)nc / 4u;
            f.C = C;
            f.dL_dfeatures = dL_dfeatures;
            const size_t blocks = ((size_t)P * f.cq + 255) / 256;
            if (blocks > 0x7fffffffull) throw Error("feature_maps_backward: P * C is too large for one launch");
            hipLaunchKernelGGL(feat_bwd_feature_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, f);
            check_launch("feature maps backward, feature sums", s, false);
        }
        if (geom) {
            FeatGaussArgs g;
            g.rec = st.geom.rec;
            g.radii = radii;
            g.tiles = st.geom.tiles;
            g.keys = w.keys_out;
            g.slots = w.slots_out;
            g.slab_g = w.slab_g;
            g.view = viewmatrix;
            g.proj = projmatrix;
            g.means3D = means3D;
            g.scales = scales;
            g.rotations = rotations;
            g.cov3D_precomp = cov3D_precomp;
            g.tan_fovx = tan_fovx;
            g.tan_fovy = tan_fovy;
            g.scale_modifier = scale_modifier;
            g.W = width;
            g.H = height;
            g.P = (uint32_t)P;
            g.R = (uint32_t)R;
            g.ngroups = a.ngroups;
            g.dL_dmeans2D = dL_dmeans2D;
            g.dL_dmeans3D = dL_dmeans3D;
            g.dL_dopacity = dL_dopacity;
            g.dL_dscales = dL_dscales;
            g.dL_drotations = dL_drotations;
            g.dL_dcov3D = dL_dcov3D;
            const uint32_t gblocks = ((uint32_t)P + 63u) / 64u;
            if (g_f64_chain.get())
                hipLaunchKernelGGL(feat_bwd_gauss_kernel<true>, dim3(gblocks), dim3(64), 0, s, g);
            else
                hipLaunchKernelGGL(feat_bwd_gauss_kernel<false>, dim3(gblocks), dim3(64), 0, s, g);
            check_launch("feature maps backward, per-Gaussian chain", s, false);
        }
        return 0;
    });
}

}  // extern "C"
