// block_scan.h -- the workgroup primitives of the model-state units (densify.hip, mcmc.hip): wave64,
// kScanBlock threads, every thread of the workgroup calls.  LDS rows are the caller's: kScanWaves elements per scanned or
// counted quantity.  No atomics; the order of every addition is fixed, so float sums are the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>

namespace r3 {

constexpr int kScanBlock = 256;
constexpr int kScanWaves = kScanBlock / 64;
constexpr int kScanSpan = kScanBlock;   // plan workgroups the one scan workgroup takes per round (= 65536 Gaussians)

// The tree of the inclusive scan, in two halves around ONE barrier of the caller's (so that scans can share it):
// shuffle-up inside the wave, the wave's total into s_wave; then the totals of the waves summed in wave order.  The double
// cdf of mcmc.hip depends on exactly this order of additions.
template <typename T>
__device__ __forceinline__ T scan_publish(T x, T* s_wave)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    return x;
}
template <typename T>
__device__ __forceinline__ T scan_combine(T x, const T* s_wave, T& total)
{
    const int wave = threadIdx.x >> 6;
    T before = T(0), all = T(0);
#pragma unroll
    for (int w = 0; w < kScanWaves; w++) {
        const T s = s_wave[w];
        before += w < wave ? s : T(0);
        all += s;
    }
    total = all;
    return before + x;
}
// -> the thread's inclusive value; total: the workgroup's.
template <typename T>
__device__ __forceinline__ T block_scan(T x, T* s_wave, T& total)
{
    x = scan_publish(x, s_wave);
    __syncthreads();
    return scan_combine(x, s_wave, total);
}

// counts[k] = the threads of the workgroup with flag[k]: ballot, popcount, LDS sum over the waves; thread k < K writes.
template <int K>
__device__ __forceinline__ void block_count(const bool (&flag)[K], int (&s_count)[K][kScanWaves], int* __restrict__ counts)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n[K];
#pragma unroll
    for (int k = 0; k < K; k++) n[k] = (int)__popcll(__ballot(flag[k]));
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) s_count[k][wave] = n[k];
    }
    __syncthreads();
    if (tid < K) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) sum += s_count[tid][w];
        counts[tid] = sum;
    }
}

// rank[k] = the threads of the workgroup below this one with flag[k]: lanes below in the wave, waves below in the workgroup.
// Added to the workgroup's scanned offset it is the stable rank of a flagged thread: rows come out in source order.
template <int K>
__device__ __forceinline__ void block_rank(const bool (&flag)[K], int (&s_count)[K][kScanWaves], int (&rank)[K])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const unsigned long long m = __ballot(flag[k]);
        rank[k] = __popcll(m & below);
        if (lane == 0) s_count[k][wave] = __popcll(m);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) rank[k] += w < wave ? s_count[k][w] : 0;
    }
}

// One round of the scan workgroup over rows of K per-workgroup counts, in two halves around one barrier of the caller's.
// The thread takes row b (none past nb); the carries of the rounds before live in every thread's registers.
template <int K>
__device__ __forceinline__ void scan_round_publish(const int* __restrict__ counts, long long b, long long nb, int (&v)[K],
                                                   int (&inc)[K], int (&s_wave)[K][kScanWaves])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        v[k] = b < nb ? counts[b * K + k] : 0;
        inc[k] = scan_publish(v[k], s_wave[k]);
    }
}
// -> excl[k]: the exclusive offset of row b over all rounds; carry[k] takes the round's total.
template <int K>
__device__ __forceinline__ void scan_round_combine(const int (&v)[K], const int (&inc)[K], const int (&s_wave)[K][kScanWaves],
                                                   int (&carry)[K], int (&excl)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        int all;
        excl[k] = carry[k] + scan_combine(inc[k], s_wave[k], all) - v[k];
        carry[k] += all;
    }
}

}  // namespace r3
