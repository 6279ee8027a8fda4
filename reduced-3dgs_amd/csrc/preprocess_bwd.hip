// preprocess_bwd.hip -- per-Gaussian backward stage on gfx950, ONE fused kernel.
//
// Replaces the two reference kernels cuda_rasterizer/backward.cu:177-307 computeCov2DCUDA and
// backward.cu:379-434 preprocessCUDA (+ :20-172 SH, :311-374 cov3D), and the count(radii>0) reduction of
// rasterizer_impl.cu:549-571 (the visible count was already produced by the forward; no host sync, no
// malloc/free in the backward) of /root/reference/submodules/diff-gaussian-rasterization.
//
// The 2D-stage gradients arrive as one 9-float row per (tile, Gaussian) pair; pair_reduce_kernel below sums
// them per Gaussian first (segmented sum, no atomics).
// HBM-bound streaming kernel: one lane per Gaussian.  The wave's 64 SH rows are staged through LDS with
// coalesced loads, the dL/dsh rows are built IN PLACE in the same LDS span and written back with
// coalesced stores -- including the zeros the API contract demands for bands above a Gaussian's degree
// and for culled Gaussians -- so the caller does not have to memset the 12*M*P-byte tensor first.
// Every output element of every Gaussian is written (zeros where the reference leaves its
// zero-initialised tensors untouched), so outputs may be uninitialised memory.
#include "common.h"
#include "sh_rows.h"

namespace r3 {

// Workgroup size of preprocess_bwd_kernel.  One wave per workgroup (round 4): every wave owns its LDS window and its 64
// Gaussians anyway, and without a four-wave barrier the twelve waves of a CU drift apart, so loads, evaluation and the
// dL_dsh row stores of different waves overlap: 0.194 -> 0.181 ms at 2 M Gaussians, 0.574 -> 0.539 at 6 M, unchanged at
// 500 k (0.062-0.064 either way); 128: in between.
constexpr int kBwdBlock = 64;

// ------------------------------------------------------------------------------------------------
// Per-Gaussian sums of the per-(tile, Gaussian)-pair gradients written by the backward blend.
// The slab is in emission order, i.e. a Gaussian's pairs are contiguous, so this is a segmented sum over a
// sorted key (the Gaussian id of each pair = the unsorted value array of the tile sort).  One lane per pair,
// coalesced loads, a 6-step segmented scan inside each wave.  A run that lies inside one 64-pair group is
// final and goes to acc[gid]; a run cut by a group boundary leaves its piece in the group's
// leading / trailing slot and the per-Gaussian kernel adds the <= (tiles/64 + 2) pieces in order.
// No atomics, fixed summation order: the backward is bit-reproducible.  (Letting each Gaussian's lane loop
// over its own pairs instead cost 0.86 ms: the largest splats own 600+ pairs.)
// ------------------------------------------------------------------------------------------------
constexpr int kReduceGroups = 1;   // 64-pair groups per wave and trip (2, with all their loads in flight together, measured the
                                   // same 49 us: the kernel moves whole 128-byte lines of the slab for the ~45 % of its 48-byte
                                   // rows that are flagged, ~3.6 TB/s of DRAM traffic)

// segmented sum of one 64-pair group (one pair per lane) and the stores of its run totals
__device__ __forceinline__ void pair_reduce_group(const PairReduceArgs& a, uint32_t e, int lane, bool valid, uint32_t key,
                                                  float (&v)[kPairGrad], uint32_t key_before, uint32_t key_after)
{
    // Inclusive segmented scan over equal-key runs, on DPP (VALU) moves only: Kogge-Stone inside each row of 16 lanes
    // (row_shr 1, 2, 4, 8), then the classic row_bcast:15 / row_bcast:31 pair carries the row totals across -- valid
    // for a SEGMENTED scan because runs are contiguous: a lane shares the key of the broadcast lane iff its run reaches
    // back to it.  The first version went through ds_bpermute (60 LDS-pipe instructions per wave: 61% issue stall).
    // A lane without a source keeps `old`: ~key for the key (never equal), so it takes nothing.
#define R3_SEG_STEP(CTRL, RMASK)                                                                                          \
    {                                                                                                                     \
        const uint32_t ku = (uint32_t)__builtin_amdgcn_update_dpp((int)~key, (int)key, CTRL, RMASK, 0xf, false);          \
        const bool take = ku == key;                                                                                      \
        _Pragma("unroll") for (int k = 0; k < kPairGrad; k++)                                                             \
        {                                                                                                                 \
            const float vu = __builtin_bit_cast(                                                                          \
                float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[k]), CTRL, RMASK, 0xf, false));           \
            if (take) v[k] += vu;                                                                                         \
        }                                                                                                                 \
    }
    R3_SEG_STEP(0x111, 0xf)   // row_shr:1
    R3_SEG_STEP(0x112, 0xf)   // row_shr:2
    R3_SEG_STEP(0x114, 0xf)   // row_shr:4
    R3_SEG_STEP(0x118, 0xf)   // row_shr:8
    R3_SEG_STEP(0x142, 0xa)   // row_bcast:15 -> rows 1 and 3
    R3_SEG_STEP(0x143, 0xc)   // row_bcast:31 -> rows 2 and 3
#undef R3_SEG_STEP
    const uint32_t knext = (uint32_t)__shfl_down((int)key, 1);
    const uint32_t key0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);   // the group's first run (all lanes active here)
    if (valid && (lane == 63 || knext != key)) {  // last lane of a run: holds the run's sum inside this group
        const uint32_t gid = a.order ? global_ptr(a.order)[key] : key;
        // does the run reach across the borders of this group?  The neighbouring pairs' keys say so (runs are contiguous:
        // same key <=> same run); asking the Gaussian's record for its pair range was a dependent gather per run
        const bool from_before = key == key0 && key_before == key;
        const bool into_next = lane == 63 && key_after == key;
        if (!from_before && !into_next) {
            auto* dst = reinterpret_cast<R3_GLOBAL float4*>(global_ptr(a.acc) + (size_t)gid * kAccStride);   // 48-B row: three 16-B stores
            // A run without a contributing pair (all nine sums exactly zero: a third of the visible Gaussians of the metric scene,
            // more in a densified one) stores nothing: the reader takes a row that does not carry THIS pass's stamp for zeros.
            // 40-54 % of this kernel is these scattered stores (profiles/r06_exp_pair_reduce_stores.txt); pair_reduce 41 -> 39 us
            // at 500 k, 127 -> 92 at 2 M, 282 -> 187 at 6 M.
            bool nz = false;
#pragma unroll
            for (int k = 0; k < kPairGrad; k++) nz |= v[k] != 0.f;
            if (nz) {
                dst[0] = make_float4(v[0], v[1], v[2], v[3]);
                dst[1] = make_float4(v[4], v[5], v[6], v[7]);
                dst[2] = make_float4(v[8], __uint_as_float(a.stamp0), __uint_as_float(a.stamp1), 0.f);
            }
        } else {
            R3_GLOBAL float* wp = global_ptr(a.wave_part) + (size_t)(e >> 6) * 2 * kPieceStride;
            if (from_before) {  // continues a run of the previous group: this group's leading piece
#pragma unroll
                for (int k = 0; k < kPairGrad; k++) wp[k] = v[k];
            }
            if (into_next) {  // continues into the next group: trailing piece
#pragma unroll
                for (int k = 0; k < kPairGrad; k++) wp[kPieceStride + k] = v[k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void pair_reduce_kernel(const PairReduceArgs* __restrict__ ap)
{
    const PairReduceArgs a = *ap;
    const uint32_t R = global_ptr(a.hdr)->num_pairs;
    constexpr uint32_t kPerBlock = 256u * kReduceGroups;
  for (uint32_t blk = blockIdx.x; blk * kPerBlock < R; blk += gridDim.x) {   // logical blocks strided over the grid (common.h)
    const R3_GLOBAL float* __restrict__ pair_grad = global_ptr(a.pair_grad);
    R3_GLOBAL unsigned char* __restrict__ pair_flag = global_ptr(a.pair_flag);
    const R3_GLOBAL uint32_t* __restrict__ pair_gid = global_ptr(a.pair_rank);
    const uint32_t rank_mask = a.rank_mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t e0 = blk * kPerBlock + (uint32_t)wave * (64u * kReduceGroups) + (uint32_t)lane;
    float v[kReduceGroups][kPairGrad];
    uint32_t key[kReduceGroups], kb[kReduceGroups], ka[kReduceGroups];
    bool flag[kReduceGroups];
    // every load of the wave's groups is issued before the first use: keys, flags, neighbours' keys, then the rows
#pragma unroll
    for (int g = 0; g < kReduceGroups; g++) {
        const uint32_t e = e0 + 64u * g, gbase = e & ~63u;
        key[g] = e < R ? pair_gid[e] & rank_mask : 0xFFFFFFFFu;   // run key: the Gaussian id
        flag[g] = e < R && pair_flag[e] != 0;
        kb[g] = gbase > 0u && gbase < R ? pair_gid[gbase - 1u] & rank_mask : 0xFFFFFFFFu;
        ka[g] = gbase + 64u < R ? pair_gid[gbase + 64u] & rank_mask : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int g = 0; g < kReduceGroups; g++) {
        const uint32_t e = e0 + 64u * g;
#pragma unroll
        for (int k = 0; k < kPairGrad; k++) v[g][k] = 0.f;
        if (flag[g]) {  // ~1/3 of the pairs contribute; the rest of the slab is stale memory, never read
            pair_flag[e] = 0;  // consumed: all flags are zero again when this kernel ends (next backward pass)
            const auto* src = reinterpret_cast<const R3_GLOBAL float4*>(pair_grad + (size_t)e * kPairStride);
            const float4 r0 = src[0], r1 = src[1];
            v[g][0] = r0.x; v[g][1] = r0.y; v[g][2] = r0.z; v[g][3] = r0.w;
            v[g][4] = r1.x; v[g][5] = r1.y; v[g][6] = r1.z; v[g][7] = r1.w;
            v[g][8] = src[2].x;
        }
    }
#pragma unroll
    for (int g = 0; g < kReduceGroups; g++) {
        const uint32_t e = e0 + 64u * g;
        pair_reduce_group(a, e, lane, e < R, key[g], v[g], kb[g], ka[g]);
    }
  }
}

void issue_pair_reduce(const BwdPlan& p, const PairReduceArgs* a, hipStream_t s)
{
    if (!p.has_pairs) return;
    constexpr uint32_t per = 256u * kReduceGroups;
    hipLaunchKernelGGL(pair_reduce_kernel, dim3((p.grid_pairs + per - 1u) / per), dim3(256), 0, s, a);
}

// F64: the covariance chain in double (gauss_math.h cov2d_backward_f64 / cov3d_backward_f64; the default)
// RAW (r3dgs_backward_params): in.scales / in.rotations hold the model's raw parameters -- activated after the load, and
// dL_dscale / dL_drot, formed and rounded to fp32 exactly as without RAW, pass through the fp32 activation backward of
// param_math.h before the store; the SH rows come from in.shs (features_dc) / shs_rest and their gradient rows leave as
// out.dL_dsh / dL_dsh_rest.
template <bool ROWS48, bool F64, bool RAW = false>
__global__ __launch_bounds__(kBwdBlock) void preprocess_bwd_kernel(const PreBwdArgs* __restrict__ ap)
{
    __shared__ float s_sh[kBwdBlock / 64][kWaveShFloats];
    const PreBwdArgs a = *ap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = a.in.P, M = a.in.M;
    const int i = blockIdx.x * kBwdBlock + tid;
    const bool valid = i < P;
    const int wave_first = blockIdx.x * kBwdBlock + wave * 64;
    // Every pointer of the block goes through global_ptr() (common.h): as FLAT accesses the loads below counted on the LDS
    // counter too and each of the kernel's 24 waits drained both counters; as GLOBAL ones the camera and the header words are
    // scalar loads, and the waits for the LDS rows leave the memory loads in flight.
    const Camera cam = load_camera_from(global_ptr(a.view.view), global_ptr(a.view.proj), global_ptr(a.view.campos), a.view);
    const bool has_sh = a.in.shs != nullptr;
    const auto* hdr = global_ptr(a.header);
    const uint32_t num_pairs = hdr->num_pairs, n_visible = hdr->visible, hdr_sh_cache = hdr->sh_cache;   // wave-uniform
    // the forward left the SH direction derivatives and there is no sparsity term: the SH rows are not read at all
    const bool cached = has_sh && a.sh_ddir != nullptr && hdr_sh_cache != 0u;

    // ---- load phase: every input of lane i whose address is a function of i alone is requested here, before the first use
    // of any of them, so that a lane pays one round trip to memory behind `radii` instead of the chain record -> pair count -> acc row
    // -> scales / rotations -> degree -> direction derivatives (eight dependent trips, each behind a full drain).  The tests
    // that used to guard the loads are applied to the loaded values below.  Left where they were: the wave_part pieces of a
    // run that spans several 64-pair groups (their address comes out of the record: the one dependent load), and the SH rows
    // of the row-reading path (a wave's staging loop, issued behind these loads).  The derivatives wait for the header word
    // that says whether the blob holds them (a blob without them ends in front of that array).
    // Culled lanes: radii first and the rest for the visible lanes only -- two trips, no byte read for a culled Gaussian.
    // Loading everything for every lane i < P at once (one trip, ~20 % more bytes read at the metric shape, 180 B instead of 4
    // per culled Gaussian) measured equal at 500 k and 2 M (profiles/prebwd_loads.txt); a view of a trained scene culls most
    // of its Gaussians, so the form that reads nothing for them is the one built.
    // (The arrays and the record stay uninitialised on the lanes that load nothing -- they are read only where `vis` holds:
    // merged with constants, the compiler copies each loaded register at the end of the phase, which waits for all of them.)
    int radius = 0, deg = 0;
    uint32_t ntile = 0u;
    GRec r;
    float4 a0, a1, a2;
    float m3[3], sc[3], q[4], c6[6], d9in[9];
    const auto load_lane = [&]() {
        r = global_ptr(a.rec)[i];
        ntile = global_ptr(a.tiles)[i];
        const auto* arow = reinterpret_cast<const R3_GLOBAL float4*>(global_ptr(a.acc) + (size_t)i * kAccStride);
        a0 = arow[0];
        a1 = arow[1];
        a2 = arow[2];
        for (int k = 0; k < 3; k++) m3[k] = global_ptr(a.in.means3D)[3 * i + k];
        if (!a.in.cov3D_precomp) {
            for (int k = 0; k < 3; k++) sc[k] = global_ptr(a.in.scales)[3 * i + k];
            for (int k = 0; k < 4; k++) q[k] = global_ptr(a.in.rotations)[4 * i + k];
        }
        if (has_sh) deg = global_ptr(a.in.degrees)[i];
        if (cached) {
#pragma unroll
            for (int k = 0; k < 9; k++) d9in[k] = global_ptr(a.sh_ddir)[9 * (size_t)i + k];
        }
        if (a.in.cov3D_precomp) {   // (a block of its own and the last one: the registers of its six words are free on the other
                                    // path, and a load issued behind a block that reused one would wait for every load before it)
            for (int k = 0; k < 6; k++) c6[k] = global_ptr(a.in.cov3D_precomp)[6 * i + k];
            sc[0] = sc[1] = sc[2] = 0.f;
            q[0] = 1.f;
            q[1] = q[2] = q[3] = 0.f;
        }
    };
    if (valid) radius = global_ptr(a.radii)[i];
    const bool vis = valid && radius > 0;
    if (vis) load_lane();

    const int nrows = max(0, min(64, P - wave_first));
    const int span_len = has_sh ? nrows * 3 * M : 0;
    const long span_first = 3L * M * wave_first;
    float* lds = s_sh[wave];
    const bool wave_vis = __ballot(vis) != 0ull;
    // The workgroups that start together (three per CU) would load their SH rows together, compute together and store
    // together: HBM idle while they compute, the SIMDs idle while they wait.  The second and third of a CU start a step
    // later each.  (Only when the rows are read: without that phase the stagger costs 2 us instead of saving 4.)
    if (!cached && a.stagger > 0 && blockIdx.x < 768u * (256 / kBwdBlock)) {
        const int steps = (int)(blockIdx.x / (256u * (256 / kBwdBlock))) * a.stagger;
        for (int k = 0; k < steps; k += 127) __builtin_amdgcn_s_sleep(127);
    }
    // sh_rows.h: the window's layout and the copies.  Six dwordx4 loads per lane in flight before the first LDS store
    // (twelve, as in the forward's colour kernel, cost a wave of occupancy).
    if (RAW) {
        if (wave_vis && !cached) stage_split_rows<ROWS48>(global_ptr(a.in.shs), global_ptr(a.shs_rest), wave_first, nrows, M, lds, lane);
    } else if (has_sh && wave_vis && !cached) {
        stage_span<6>(global_ptr(a.in.shs), span_first, span_len, ROWS48, lds, lane);
    }
    __syncthreads();

    float dmean[3] = {0.f, 0.f, 0.f}, dcov6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dscale[3] = {0.f, 0.f, 0.f}, dq[4] = {0.f, 0.f, 0.f, 0.f};
    float g2x = 0.f, g2y = 0.f, dop = 0.f, dcol[3] = {0.f, 0.f, 0.f}, gcon[3] = {0.f, 0.f, 0.f};
    int K = 0;
    const ShRow<ROWS48, float> row = sh_row<ROWS48>(lds, lane, lane * 3 * M);
    if (vis) {
        const float mx = m3[0], my = m3[1], mz = m3[2];
        // 2D-stage gradient row: final in acc[], or in <= tiles/64 + 2 ordered pieces.  A Gaussian whose pairs did not
        // all fit the pass's pair reservation (num_rendered > reserve: the farthest pairs were dropped and the pass is
        // flagged) gets zero 2D-stage gradients instead of a partial sum.
        const uint32_t start = r.pair_start;
        if (a.wave_part && start != 0xFFFFFFFFu && start + ntile <= num_pairs) {
            float acc9[kPairGrad];
            const uint32_t last = start + ntile - 1u;
            const uint32_t w0 = start >> 6, w1 = last >> 6;
            if (w0 == w1) {
                if (__float_as_uint(a2.y) != a.stamp0 || __float_as_uint(a2.z) != a.stamp1)   // not written by this pass: zeros
                    a0 = a1 = a2 = make_float4(0.f, 0.f, 0.f, 0.f);
                acc9[0] = a0.x; acc9[1] = a0.y; acc9[2] = a0.z; acc9[3] = a0.w;
                acc9[4] = a1.x; acc9[5] = a1.y; acc9[6] = a1.z; acc9[7] = a1.w;
                acc9[8] = a2.x;
            } else {   // the one dependent load of the kernel: which groups hold the run's pieces comes out of the record
                const R3_GLOBAL float* wave_part = global_ptr(a.wave_part);
                const R3_GLOBAL float* wp = wave_part + (size_t)w0 * 2 * kPieceStride + kPieceStride;  // trailing piece of w0
#pragma unroll
                for (int k = 0; k < kPairGrad; k++) acc9[k] = wp[k];
                for (uint32_t w = w0 + 1; w <= w1; w++) {  // leading piece of every following group
                    wp = wave_part + (size_t)w * 2 * kPieceStride;
#pragma unroll
                    for (int k = 0; k < kPairGrad; k++) acc9[k] += wp[k];
                }
            }
            g2x = acc9[0];
            g2y = acc9[1];
            gcon[0] = acc9[2];
            gcon[1] = acc9[3];
            gcon[2] = acc9[4];
            dop = acc9[5];
            dcol[0] = acc9[6];
            dcol[1] = acc9[7];
            dcol[2] = acc9[8];
        }
        float qn = 1.f;   // RAW: norm of the raw quaternion
        if (!a.in.cov3D_precomp) {
            if (RAW) {
                const float rq[4] = {q[0], q[1], q[2], q[3]};
                for (int k = 0; k < 3; k++) sc[k] = scale_act(sc[k]);
                qn = quat_act(rq, q);
            }
            cov3d_from_scale_rot(sc, cam.scale_modifier, q, c6);  // recomputed, not stored by the forward
        }
        double dcov6d[6];
        if (F64) {
            cov2d_backward_f64(cam, mx, my, mz, c6, gcon[0], gcon[1], gcon[2], dcov6d, dmean);
#pragma unroll
            for (int k = 0; k < 6; k++) dcov6[k] = (float)dcov6d[k];
        } else {
            cov2d_backward(cam, mx, my, mz, c6, gcon[0], gcon[1], gcon[2], dcov6, dmean);
        }
        project_backward(cam, mx, my, mz, g2x, g2y, dmean);
        if (has_sh) {
            float mult = 0.f;
            if (a.lambda_sh != 0.f) mult = a.lambda_sh / (float)((int)n_visible * 15 * 3);
            K = (deg + 1) * (deg + 1);
            if (cached) {
                float d9[9];
#pragma unroll
                for (int k = 0; k < 9; k++)   // (a Gaussian binned into no tile got no colour and left nothing: its dcol is 0)
                    d9[k] = (deg > 0 && ntile > 0u) ? d9in[k] : 0.f;
                sh_backward<true>(deg, row, row, d9, mx, my, mz, cam.campos, r.width_clamp >> 16, dcol, 0.f, dmean);
            } else {
                sh_backward<false>(deg, row, row, nullptr, mx, my, mz, cam.campos, r.width_clamp >> 16, dcol, mult, dmean);
            }
        }
        if (a.in.scales) {
            if (F64)
                cov3d_backward_f64(sc, cam.scale_modifier, q, dcov6d, dscale, dq);
            else
                cov3d_backward(sc, cam.scale_modifier, q, dcov6, dscale, dq);
            if (RAW) {   // gradients of the activated values (fp32, as stored without RAW) -> gradients of the raw parameters
                for (int k = 0; k < 3; k++) dscale[k] = scale_act_bwd(dscale[k], sc[k]);
                const float gq[4] = {dq[0], dq[1], dq[2], dq[3]};
                quat_act_bwd(q, qn, gq, dq);
            }
        }
        dop = opacity_backward(dop, r.op);
    }
    if (has_sh && valid) {
        if (wave_vis) {
            for (int e = 3 * K; e < 3 * M; e++) row.put(e, 0.f);  // bands above this Gaussian's degree / culled rows
        }
    }
    __syncthreads();
    // the gradient rows (or zeros) leave the way the rows came
    if (RAW)
        unstage_split_rows<ROWS48>(global_ptr(a.out.dL_dsh), global_ptr(a.dL_dsh_rest), wave_first, nrows, M, lds, lane, wave_vis);
    else if (has_sh)
        unstage_span<ROWS48>(global_ptr(a.out.dL_dsh), span_first, span_len, lds, lane, wave_vis);
    if (valid) {
        R3_GLOBAL float* o;
        o = global_ptr(a.out.dL_dmean2D) + 3 * (size_t)i;
        o[0] = g2x;
        o[1] = g2y;
        o[2] = 0.f;
        global_ptr(a.out.dL_dopacity)[i] = dop;
        o = global_ptr(a.out.dL_dcolor) + 3 * (size_t)i;
        o[0] = dcol[0];
        o[1] = dcol[1];
        o[2] = dcol[2];
        o = global_ptr(a.out.dL_dmean3D) + 3 * (size_t)i;
        o[0] = dmean[0];
        o[1] = dmean[1];
        o[2] = dmean[2];
        o = global_ptr(a.out.dL_dcov3D) + 6 * (size_t)i;
        for (int k = 0; k < 6; k++) o[k] = dcov6[k];
        o = global_ptr(a.out.dL_dscale) + 3 * (size_t)i;
        o[0] = dscale[0];
        o[1] = dscale[1];
        o[2] = dscale[2];
        o = global_ptr(a.out.dL_drot) + 4 * (size_t)i;
        o[0] = dq[0];
        o[1] = dq[1];
        o[2] = dq[2];
        o[3] = dq[3];
        if (a.out.dL_dconic) {
            o = global_ptr(a.out.dL_dconic) + 4 * (size_t)i;
            o[0] = gcon[0];
            o[1] = gcon[1];
            o[2] = 0.f;
            o[3] = gcon[2];
        }
    }
}

void issue_preprocess_backward(const BwdPlan& p, const PreBwdArgs* a, hipStream_t s)
{
    const int blocks = (p.P + kBwdBlock - 1) / kBwdBlock;
    static const int lds_pad = env_int("R3DGS_PREBWD_LDS_PAD", 0, 0, 65536);
    if (p.raw_params) {
        if (p.M == 16) {
            if (p.f64_chain)
                hipLaunchKernelGGL((preprocess_bwd_kernel<true, true, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
            else
                hipLaunchKernelGGL((preprocess_bwd_kernel<true, false, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
        } else {
            if (p.f64_chain)
                hipLaunchKernelGGL((preprocess_bwd_kernel<false, true, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
            else
                hipLaunchKernelGGL((preprocess_bwd_kernel<false, false, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
        }
        return;
    }
    if (p.M == 16) {
        if (p.f64_chain)
            hipLaunchKernelGGL((preprocess_bwd_kernel<true, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
        else
            hipLaunchKernelGGL((preprocess_bwd_kernel<true, false>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
    } else {
        if (p.f64_chain)
            hipLaunchKernelGGL((preprocess_bwd_kernel<false, true>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
        else
            hipLaunchKernelGGL((preprocess_bwd_kernel<false, false>), dim3(blocks), dim3(kBwdBlock), lds_pad, s, a);
    }
}

}  // namespace r3
