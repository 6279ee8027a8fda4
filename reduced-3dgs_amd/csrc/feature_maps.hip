// feature_maps.hip -- a per-Gaussian feature vector F[P, C] blended into a [C, H, W] map, and the gradients through it
// (include/r3dgs_features.h; the arithmetic is feature_math.h), gfx950.  Replay passes (DESIGN.md "Replay passes"; the
// walk's shared part is replay_walk.h): they read the three state blobs and write only the caller's outputs and workspace.
//
// Channels go in register-resident groups of NC = 4, 8 or 16 (the smallest that holds C, 16 beyond); a map of more channels
// than a group is a further walk per group, over the second grid dimension: one wave per (quadrant, channel group).
//
// Forward, feat_fwd_kernel<NC> -- the walk front to back: lane j gathers, beside the record of entry j, the group's slice of
// its feature row (16-byte loads when the rows allow it) and parks NC floats beside the record in LDS, 6 KB per workgroup at
// NC = 16; the step is the forward's own (feature_math.h feat_step).  Plain vector stores; a partial tile writes only the
// pixels inside the image.
//
// Backward, four or five launches on the caller's stream (the route of aux_bwd.hip; no host wait, no allocation, no atomics):
//   1. feat_bwd_pixel_kernel<NC, GEOM, FEAT> -- the walk back to front with T recovered from final_T by
//      division.  Per entry some lane blended, the wave reduces the group's NC channel sums and (GEOM) the six geometric
//      sums with a TRANSPOSING reduction: at every step a lane hands half of its values to its partner and keeps the sums
//      of the other half, so N values cost N - 1 + (6 - log2 N) shuffles instead of 6 N, and lane l ends up with the
//      whole-wave sum of value feat_sum_slot(l).  Per chunk, lane j stores the rows of entry j -- the sums, or zeros for an
//      entry no lane blended -- at (list slot, quadrant[, group]); the slots behind the walk get zero rows.  Every row of
//      every slot < num_pairs is written in every call by exactly one wave: the slabs need no clearing.
//      The backward's recurrence is linear in the channels: each group carries its own and their geometric sums add up.
//   2, 3. the (Gaussian id, list slot) keys and their stable sort by id (pair_sort.h).
//   4. feat_bwd_feature_kernel -- one lane per (Gaussian, four channels): its run of the sorted keys, its rows added in
//      sorted order (slot ascending, quadrant 0..3) in double -> dL_dfeatures.
//   5. feat_bwd_gauss_kernel<F64> (GEOM) -- one lane per Gaussian: the six sums over (slot, quadrant, group) in double, then
//      aux_bwd.hip's per-Gaussian tail (aux_bwd_stage.h) with a zero z sum.
// A Gaussian that lost pairs to an overflowed reservation (its run is shorter than its tiles_touched) gets zero rows.
// The order of every sum is fixed by the data alone: the results are bit-identical run to run.
// Workspace per pair, G = ceil(C / 16) groups (NC = 16): 4 x G x 64 B feature rows + 4 x G x 32 B geometric rows + 16 B of
// keys and slots = 384 G + 16 bytes, plus rocPRIM's temp storage.
#include <string>

#include "../../include/r3dgs_features.h"
#include "aux_bwd_stage.h"
#include "feature_math.h"
#include "common.h"
#include "pass_driver.h"

namespace r3 {

namespace {

constexpr int kGeoRow = 8;   // floats per geometric row: sx, sy, sxx, sxy, syy, sm, 0, 0

// (the staged record's own words: b.z unused, b.w the 1-based list position in the forward)
struct FeatArgs : WalkArgs {
    const float* features;   // [P, C]
    const float* g_out;      // backward: dL_dout [C, H*W]
    int C;
    int vec4;                // the feature rows can be read as float4 (C % 4 == 0 and a 16-byte aligned base)
    uint32_t ngroups;
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
__device__ __forceinline__ void park_slice(float4 (*s_feat)[kWalkChunk], int lane, const float (&f)[NC])
{
#pragma unroll
    for (int q = 0; q < NC / 4; q++) s_feat[q][lane] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
}

template <int NC>
__device__ __forceinline__ void read_slice(const float4 (*s_feat)[kWalkChunk], int j, float (&f)[NC])
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

template <int NC>
__global__ __launch_bounds__(64) void feat_fwd_kernel(const FeatArgs a)
{
    __shared__ WalkRec s_rec[kWalkChunk];
    __shared__ float4 s_feat[NC / 4][kWalkChunk];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const int c0 = (int)blockIdx.y * NC;
    const WalkSpan sp = load_walk_span(a, q);
    const uint32_t first = sp.first, end = sp.first + sp.len;
    const float pxf = q.pxf, pyf = q.pyf;
    const bool inside = q.inside;
    const size_t pix = q.pix;
    const uint32_t n = inside ? global_ptr(a.n_contrib)[pix] : 0u;
    FeatPix<NC> p;
    feat_pix_init<NC>(p, inside);

    // software pipeline: the records of chunk k+1 are gathered into registers while chunk k is walked
    float nxf[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) nxf[c] = 0.f;
    auto gather = [&](uint32_t idx) {
        const WalkGather g = gather_rec(a.point_list, a.rec, a.P, idx, end);
        if (g.have) load_slice<NC>(a, g.id, c0, nxf);
        return g;
    };
    WalkGather nx = gather(first + (uint32_t)lane);
    for (uint32_t base = first; base < end; base += kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, 0.f, __uint_as_float(base - first + (uint32_t)lane + 1u));
        park_slice<NC>(s_feat, lane, nxf);
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        nx = gather(base + kWalkChunk + (uint32_t)lane);
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            float f[NC];
            read_slice<NC>(s_feat, j, f);
            feat_step<NC>(load_splat(s_rec[j]), pxf, pyf, load_pos1(s_rec[j]), n, f, p);
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
    __shared__ WalkRec s_rec[kWalkChunk];
    __shared__ float4 s_feat[GEOM ? NC / 4 : 1][kWalkChunk];
    __shared__ float s_outf[FEAT ? kWalkChunk : 1][NC];
    __shared__ float s_outg[GEOM ? kWalkChunk : 1][kGeoRow];
    const int lane = threadIdx.x;
    const QuadLane q = quad_lane(xcd_remap(blockIdx.x, a.nblocks), lane, a.gx, a.W, a.H);
    const uint32_t grp = blockIdx.y;
    const int c0 = (int)grp * NC;
    const WalkSpan sp = load_walk_span(a, q);
    const uint32_t first = sp.first, list_len = sp.list_len, len = sp.len;
    const int quad = q.quad;
    const float pxf = q.pxf, pyf = q.pyf;
    const bool inside = q.inside;
    const size_t pix = q.pix;
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
    for (uint32_t k = len + (uint32_t)lane; k < list_len; k += kWalkChunk) {
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
    float nxf[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) nxf[c] = 0.f;
    auto gather = [&](uint32_t k) {   // k: position in the list
        const WalkGather g = gather_rec(a.point_list + first, a.rec, a.P, k, len);
        if (GEOM && g.have) load_slice<NC>(a, g.id, c0, nxf);
        return g;
    };
    const uint32_t cfirst = ((len - 1u) / kWalkChunk) * kWalkChunk;
    WalkGather nx = gather(cfirst + (uint32_t)lane);
    FeatSums<NC> sg;
    feat_sums_clear<NC>(sg);
    const int fslot = feat_sum_slot<NC>(lane), gslot = feat_sum_slot<kGeoRow>(lane);
    for (uint32_t cbase = cfirst;; cbase -= kWalkChunk) {
        __syncthreads();
        s_rec[lane] = stage_rec(nx.a, nx.b, 0.f, 0.f);
        if (GEOM) park_slice<NC>(s_feat, lane, nxf);
        unsigned long long mask = __ballot(nx.have && walk_pretest(nx.a, nx.b, q.qx0, q.qy0));
        __syncthreads();
        if (cbase >= kWalkChunk) nx = gather(cbase - kWalkChunk + (uint32_t)lane);
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
    gauss_grad_clear(o);
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
    gauss_grad_store(a, i, o);
}

int group_width(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : kFeatGroup; }

// the workspace: the two slabs, then the sort's arrays and temp storage
struct FeatWork {
    float *slab_f, *slab_g;
    PairSortWork sort;
    char* end;
    static FeatWork carve(char* base, size_t R, int C, size_t temp_bytes)
    {
        const size_t nc = (size_t)group_width(C), groups = ((size_t)C + nc - 1) / nc;
        Carver c(base);
        FeatWork w;
        w.slab_f = c.take<float>(R * 4 * groups * nc);
        w.slab_g = c.take<float>(R * 4 * groups * kGeoRow);
        w.sort = PairSortWork::carve(c, R, temp_bytes);
        w.end = c.p;
        return w;
    }
};

void check_dims(const char* what, int P, int R, int C, int width, int height)
{
    check_replay_dims(what, P, R, width, height);
    if (C < 1 || C > R3DGS_FEATURE_MAX_CHANNELS)
        throw Error(std::string(what) + ": need 1 <= C <= " + std::to_string(R3DGS_FEATURE_MAX_CHANNELS) + " channels, got C = " +
                    std::to_string(C));
}

FeatArgs base_args(const PassStates& st, const TileGrid& grid, int P, int R, int width, int height, const float* features, int C)
{
    const int nc = group_width(C);
    const int vec4 = (C % 4 == 0) && (reinterpret_cast<uintptr_t>(features) % 16 == 0);
    return {walk_args_of(st, grid, P, R, width, height), features, nullptr, C, vec4, (uint32_t)((C + nc - 1) / nc), nullptr, nullptr,
            nullptr};
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
        const TileGrid grid = replay_grid("feature_maps", width, height);
        const size_t N = (size_t)width * height;
        if (!out) return 0;
        if (P == 0 || R == 0) {   // nothing was binned: nothing to walk
            R3_HIP(hipMemsetAsync(out, 0, sizeof(float) * N * (size_t)C, s));
            return 0;
        }
        const PassStates st = replay_states("feature_maps", P, R, width, height, {geom_buffer, binning_buffer, image_buffer});
        if (!features) throw Error("feature_maps: features must not be NULL");
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
        out = (size_t)reinterpret_cast<uintptr_t>(FeatWork::carve(nullptr, (size_t)R, C, pair_sort_temp_bytes((size_t)R)).end) + kAlign;
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
    return r3dgs_feature_maps_backward_screen(P, R, width, height, geom_buffer, binning_buffer, image_buffer, viewmatrix,
                                              projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                                              cov3D_precomp, radii, features, C, dL_dout, dL_dfeatures, dL_dmeans2D, dL_dmeans3D,
                                              dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, nullptr, nullptr, workspace, stream);
}

int r3dgs_feature_maps_backward_screen(int P, int R, int width, int height, char* geom_buffer, char* binning_buffer,
                                       char* image_buffer, const float* viewmatrix, const float* projmatrix, float tan_fovx,
                                       float tan_fovy, const float* means3D, const float* scales, float scale_modifier,
                                       const float* rotations, const float* cov3D_precomp, const int* radii,
                                       const float* features, int C, const float* dL_dout, float* dL_dfeatures,
                                       float* dL_dmeans2D, float* dL_dmeans3D, float* dL_dopacity, float* dL_dscales,
                                       float* dL_drotations, float* dL_dcov3D, float* dL_dconic, float* dL_dz, char* workspace,
                                       void* stream)
{
    return r3::guarded_call([&]() {
        using namespace r3;
        hipStream_t s = static_cast<hipStream_t>(stream);
        // (without the two screen-space outputs this is r3dgs_feature_maps_backward itself, message for message)
        const std::string name = dL_dconic || dL_dz ? "feature_maps_backward_screen" : "feature_maps_backward";
        const AuxBwdGeom in = {viewmatrix, projmatrix, tan_fovx, tan_fovy, means3D, scales, scale_modifier, rotations,
                               cov3D_precomp, radii, dL_dmeans2D, dL_dmeans3D, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D,
                               dL_dconic, dL_dz};
        const bool geom = in.any_output();
        const bool feat = dL_dfeatures != nullptr;
        const auto walk = replay_bwd_open(
            name.c_str(), P, R, width, height, {geom_buffer, binning_buffer, image_buffer}, dL_dout != nullptr, in,
            dL_dfeatures, (size_t)C, workspace, s, [&](const char* what) { check_dims(what, P, R, C, width, height); },
            [&] {
                if (!radii) throw Error(name + ": radii must not be NULL");
                if (!geom) return;   // a frozen geometry: none of its inputs is read
                if (!features) throw Error(name + ": the geometry gradients need features");
                if (in.screen_output() && !in.model_output()) return;   // a frozen model: the screen-space sums read no more
                if (!viewmatrix || !projmatrix || !means3D)
                    throw Error(name + ": the geometry gradients need viewmatrix, projmatrix and means3D");
                if (!cov3D_precomp && (!scales || !rotations))
                    throw Error(name + ": need scales and rotations, or cov3D_precomp");
            });
        if (!walk) return 0;
        const PassStates& st = walk->st;
        const TileGrid& grid = walk->grid;
        const FeatWork w = FeatWork::carve(workspace, (size_t)R, C, pair_sort_temp_bytes((size_t)R));

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

        launch_pair_sort("feature maps backward", st, P, R, w.sort, s);

        if (feat) {
            FeatSumArgs f;
            f.radii = radii;
            f.tiles = st.geom.tiles;
            f.keys = w.sort.keys_out;
            f.slots = w.sort.slots_out;
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
        if (geom && in.screen_output()) {
            launch_screen_gauss("feature maps backward", st, w.sort, P, R, width, height, in, w.slab_g, 4u * a.ngroups, s);
        } else if (geom) {
            FeatGaussArgs g = gauss_args_of<FeatGaussArgs>(st, w.sort, P, R, width, height, in);
            g.slab_g = w.slab_g;
            g.ngroups = a.ngroups;
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
