// absgrad.hip -- per-Gaussian sums of the abs columns an ABS backward blend leaves in the per-pair slab (blend.hip; DESIGN.md
// "Absolute screen-space gradients").
//
// The blend's ABS instantiations put |dL/dmean2D| summed over a (tile, Gaussian) pair's pixels, viewport factors applied,
// into columns 9 and 10 of the pair's slab row.  A Gaussian's pairs are contiguous in the slab (emission order), so its two
// sums are a segmented sum over the run key pair_reduce_kernel uses (preprocess_bwd.hip) -- the same scan, over two columns,
// in three launches between the blend and pair_reduce, while the pair flags are still set (they are read, not cleared):
//   absgrad_clear_kernel   zeros the [P,3] output (a kernel, not a memset node: the pointer comes out of the pass block, which a
//                          replayed graph refreshes; a memset node would keep the pointer it was captured with)
//   absgrad_reduce_kernel  one lane per pair, a 6-step segmented DPP scan per 64-pair group; a run inside one group stores its
//                          sums to the output row, a run cut by a group boundary leaves its leading / trailing piece in the
//                          caller's workspace ((R / 64 + 1) groups x 2 pieces x 2 floats)
//   absgrad_finish_kernel  one lane per group boundary: the lane of the group in which a cut run STARTS adds the run's pieces
//                          in order (trailing piece of that group, leading piece of every following one) and stores the row
// No float atomics, one writer per output row, fixed summation order: bit-identical run to run.  Nothing of the default pass
// is touched: pair_reduce_kernel, the acc rows, wave_part and the blobs are as they were.
// A Gaussian whose pairs did not all fit the pass's reservation keeps its zeros, as its signed row does (preprocess_bwd.hip).
#include "common.h"

namespace r3 {

__global__ __launch_bounds__(256) void absgrad_clear_kernel(const BwdPassArgs* __restrict__ ap)
{
    R3_GLOBAL float* out = global_ptr(ap->abs.out);
    const size_t n = 3 * (size_t)ap->pre.in.P;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) out[k] = 0.f;
}

// run key -> Gaussian id, as pair_reduce_group maps it (the pass driver leaves `order` null today: the key is the id)
__device__ __forceinline__ uint32_t run_gaussian(const PairReduceArgs& a, uint32_t key)
{
    return a.order ? global_ptr(a.order)[key] : key;
}

// all of the Gaussian's pairs are inside the pass's pair count (else: truncated pass, the row stays zero)
__device__ __forceinline__ bool whole_run(const PairReduceArgs& a, uint32_t gid, uint32_t R)
{
    const uint32_t start = global_ptr(a.rec)[gid].pair_start, n = global_ptr(a.tiles)[gid];
    return start != 0xFFFFFFFFu && start + n <= R;
}

__global__ __launch_bounds__(256) void absgrad_reduce_kernel(const BwdPassArgs* __restrict__ ap)
{
    const PairReduceArgs a = ap->reduce;
    const AbsGradArgs ab = ap->abs;
    const uint32_t R = global_ptr(a.hdr)->num_pairs;
    const bool truncated = global_ptr(a.hdr)->num_rendered > R;   // wave-uniform, rare
    const R3_GLOBAL float* __restrict__ pair_grad = global_ptr(a.pair_grad);
    const R3_GLOBAL unsigned char* __restrict__ pair_flag = global_ptr(a.pair_flag);
    const R3_GLOBAL uint32_t* __restrict__ pair_gid = global_ptr(a.pair_rank);
    const uint32_t rank_mask = a.rank_mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; (uint64_t)blk * 256u < R; blk += gridDim.x) {
        const uint32_t e = blk * 256u + (uint32_t)wave * 64u + (uint32_t)lane, gbase = e & ~63u;
        const bool valid = e < R;
        const uint32_t key = valid ? pair_gid[e] & rank_mask : 0xFFFFFFFFu;
        const bool flag = valid && pair_flag[e] != 0;
        const uint32_t key_before = gbase > 0u && gbase < R ? pair_gid[gbase - 1u] & rank_mask : 0xFFFFFFFFu;
        const uint32_t key_after = gbase + 64u < R ? pair_gid[gbase + 64u] & rank_mask : 0xFFFFFFFFu;
        float v[kAbsCols] = {0.f, 0.f};
        if (flag) {   // columns 8..11 of the 48-byte row
            const float4 r2 = reinterpret_cast<const R3_GLOBAL float4*>(pair_grad + (size_t)e * kPairStride)[2];
            v[0] = r2.y;
            v[1] = r2.z;
        }
        // inclusive segmented scan over equal-key runs (as pair_reduce_group): Kogge-Stone inside each row of 16 lanes, then
        // row_bcast:15 / row_bcast:31 carry the row totals across.  A lane without a source keeps ~key: it takes nothing.
#define R3_ABS_SEG_STEP(CTRL, RMASK)                                                                                      \
    {                                                                                                                     \
        const uint32_t ku = (uint32_t)__builtin_amdgcn_update_dpp((int)~key, (int)key, CTRL, RMASK, 0xf, false);          \
        const bool take = ku == key;                                                                                      \
        _Pragma("unroll") for (int k = 0; k < kAbsCols; k++)                                                              \
        {                                                                                                                 \
            const float vu = __builtin_bit_cast(                                                                          \
                float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[k]), CTRL, RMASK, 0xf, false));           \
            if (take) v[k] += vu;                                                                                         \
        }                                                                                                                 \
    }
        R3_ABS_SEG_STEP(0x111, 0xf)   // row_shr:1
        R3_ABS_SEG_STEP(0x112, 0xf)   // row_shr:2
        R3_ABS_SEG_STEP(0x114, 0xf)   // row_shr:4
        R3_ABS_SEG_STEP(0x118, 0xf)   // row_shr:8
        R3_ABS_SEG_STEP(0x142, 0xa)   // row_bcast:15 -> rows 1 and 3
        R3_ABS_SEG_STEP(0x143, 0xc)   // row_bcast:31 -> rows 2 and 3
#undef R3_ABS_SEG_STEP
        const uint32_t knext = (uint32_t)__shfl_down((int)key, 1);
        const uint32_t key0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
        if (valid && (lane == 63 || knext != key)) {   // last lane of a run inside this group
            const bool from_before = key == key0 && key_before == key;
            const bool into_next = lane == 63 && key_after == key;
            if (!from_before && !into_next) {
                const uint32_t gid = run_gaussian(a, key);
                if (!truncated || whole_run(a, gid, R)) {
                    R3_GLOBAL float* dst = global_ptr(ab.out) + 3 * (size_t)gid;
                    dst[0] = v[0];
                    dst[1] = v[1];
                }
            } else {
                R3_GLOBAL float* wp = global_ptr(ab.workspace) + (size_t)(e >> 6) * kAbsPiece;
                if (from_before) {
                    wp[0] = v[0];
                    wp[1] = v[1];
                }
                if (into_next) {
                    wp[kAbsCols] = v[0];
                    wp[kAbsCols + 1] = v[1];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void absgrad_finish_kernel(const BwdPassArgs* __restrict__ ap)
{
    const PairReduceArgs a = ap->reduce;
    const AbsGradArgs ab = ap->abs;
    const uint32_t R = global_ptr(a.hdr)->num_pairs;
    const bool truncated = global_ptr(a.hdr)->num_rendered > R;
    const R3_GLOBAL uint32_t* __restrict__ pair_gid = global_ptr(a.pair_rank);
    const R3_GLOBAL float* __restrict__ ws = global_ptr(ab.workspace);
    const uint32_t rank_mask = a.rank_mask;
    const uint32_t groups = (uint32_t)(((uint64_t)R + 63u) >> 6);
    // group w: does a run START in it and go on into group w + 1?
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w + 1u < groups; w += gridDim.x * 256u) {
        const uint32_t last = w * 64u + 63u;                  // < R: group w + 1 exists
        const uint32_t key = pair_gid[last] & rank_mask;
        if ((pair_gid[last + 1u] & rank_mask) != key) continue;   // the run ends with this group
        if (w > 0u && (pair_gid[w * 64u] & rank_mask) == key && (pair_gid[w * 64u - 1u] & rank_mask) == key)
            continue;   // the whole group is the middle of a run that started earlier: that group's lane adds it up
        float sx = ws[(size_t)w * kAbsPiece + kAbsCols], sy = ws[(size_t)w * kAbsPiece + kAbsCols + 1];   // trailing piece
        for (uint32_t g = w + 1u;; g++) {   // leading piece of every following group the run reaches
            sx += ws[(size_t)g * kAbsPiece];
            sy += ws[(size_t)g * kAbsPiece + 1];
            const uint32_t glast = g * 64u + 63u;
            if (glast + 1u >= R) break;                                   // the list ends inside or with group g
            if ((pair_gid[glast] & rank_mask) != key || (pair_gid[glast + 1u] & rank_mask) != key) break;
        }
        const uint32_t gid = run_gaussian(a, key);
        if (truncated && !whole_run(a, gid, R)) continue;
        R3_GLOBAL float* dst = global_ptr(ab.out) + 3 * (size_t)gid;
        dst[0] = sx;
        dst[1] = sy;
    }
}

void issue_absgrad_reduce(const BwdPlan& p, const BwdPassArgs* a, hipStream_t s)
{
    const size_t n = 3 * (size_t)p.P;
    const uint32_t clear_blocks = (uint32_t)((n + 1023) / 1024 < 4096 ? (n + 1023) / 1024 : 4096);
    hipLaunchKernelGGL(absgrad_clear_kernel, dim3(clear_blocks ? clear_blocks : 1u), dim3(256), 0, s, a);
    if (!p.has_pairs) return;
    hipLaunchKernelGGL(absgrad_reduce_kernel, dim3((p.grid_pairs + 255u) / 256u), dim3(256), 0, s, a);
    const uint32_t groups = p.grid_pairs / 64u + 1u;
    hipLaunchKernelGGL(absgrad_finish_kernel, dim3((groups + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace r3
