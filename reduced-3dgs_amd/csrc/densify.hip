// densify.hip -- densification of include/r3dgs_densify.h: what the reference does with two cat passes and two mask-index
// passes over every parameter, both of its Adam moments, _degrees and the accumulators, and a dozen host waits
// (scene/gaussian_model.py:502-522, :553-691), as one read and one write of the state.  Per-Gaussian arithmetic: densify_math.h.
//
// Three phases, wave64, 256-thread workgroups, no atomics, no workgroup waits on another one:
//   plan  one lane per source Gaussian: the flag byte (clone / split / pruned itself / pruned as children), and per workgroup
//         the row counts of segments A, B, C (D has C's rows: both children share opacity and scaling) and of the clone and
//         split decisions.  prune_points(mask) takes the flags from the caller's mask instead.
//   scan  ONE workgroup walks the per-workgroup counts in rounds of kScanSpan and writes each workgroup's exclusive offsets;
//         the last thread standing writes the totals and the three statistics.  A third launch, again one lane per source
//         Gaussian, ranks the lane inside its workgroup (ballots) and writes the source index of every destination row:
//         the segments come out stable, in source order.
//   move  one launch over a table of tensors (as the Adam step's): a thread owns one 16-byte unit of a DESTINATION tensor, so
//         the stores of a wave are 1 KB contiguous; each word gathers from its source row (a row is contiguous: the lanes of
//         a 180-byte features_rest row read 180 contiguous bytes), is zero (moments and grads of new rows) or is computed from
//         the parent (xyz and scaling of the children).  A unit inside one copied row whose source address is 16-byte aligned
//         is one 16-byte load; every other unit is assembled from 4-byte loads.
// The host reads the totals once between scan and move -- it has to size the destination tensors.
// The workgroup scans, counts and ranks are block_scan.h's; the workspace carver and the tensor table row_table.h's.
#include "../../include/r3dgs_densify.h"

#include "block_scan.h"
#include "densify_math.h"
#include "row_table.h"

namespace {

constexpr int kBlock = r3::kScanBlock;
constexpr int kCounts = 5;                   // per plan workgroup: rows of A, B, C; clone and split decisions
constexpr int kSegCounts = 3;                // ... of which the first three are scanned into offsets
constexpr int kUnitWords = 4;                // a thread of the move kernel owns one 16-byte unit
constexpr int kChunkWords = kBlock * kUnitWords;
constexpr int kHeaderInts = 16;              // workspace header: the eight totals, then P
constexpr int kMaxTensors = R3DGS_DENSIFY_MAX_TENSORS;
constexpr long long kMaxP = r3::kMaxP;
using r3::plan_blocks;
static_assert(kBlock == r3::kPlanBlock && R3DGS_DENSIFY_COPY == 0, "row_table.h's grid and kind range");

struct Plan {
    int* header;      // [kHeaderInts] totals (as the caller's copy) and P: the move kernel refuses a plan that is not its own
    uint8_t* flags;   // [P]
    int* counts;      // [nb][kCounts]
    int* offsets;     // [nb][kSegCounts] exclusive, per segment
    int* map;         // [2 P] source Gaussian of every destination row (a source has at most two rows)
};
// The layout of the workspace; with ws == NULL only its size.
inline size_t carve_plan(char* ws, long long P, Plan* p)
{
    const size_t nb = (size_t)plan_blocks(P);
    r3::Carver16 c{ws};
    Plan q;
    q.header = c.take<int>(kHeaderInts);
    q.flags = c.take<uint8_t>((size_t)P);
    q.counts = c.take<int>(nb * kCounts);
    q.offsets = c.take<int>(nb * kSegCounts);
    q.map = c.take<int>(2 * (size_t)P);
    if (p) *p = q;
    return c.used();
}

// Which segments a source Gaussian has a row in.
__device__ __forceinline__ void rows_of(uint8_t f, bool in, bool& a, bool& b, bool& c)
{
    a = in && !(f & (r3::kFlagSplit | r3::kFlagPrunedSelf));
    b = in && (f & r3::kFlagClone) && !(f & r3::kFlagPrunedSelf);
    c = in && (f & r3::kFlagSplit) && !(f & r3::kFlagPrunedChild);
}

template <bool kFromMask>
__global__ __launch_bounds__(kBlock) void plan_kernel(int P, r3::DensifyThresholds t, const float* __restrict__ accum,
                                                      const float* __restrict__ denom, const float* __restrict__ scaling,
                                                      const float* __restrict__ opacity, const float* __restrict__ max_radii,
                                                      const uint8_t* __restrict__ mask, Plan out)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < P;
    uint8_t f = 0;
    if (in) {
        if constexpr (kFromMask) {
            f = mask[i] ? r3::kFlagPrunedSelf : 0;
        } else {
            const float raw[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
            const float a = t.densify ? accum[i] : 0.f, d = t.densify ? denom[i] : 1.f;
            const float radii = (!t.densify && t.screen) ? max_radii[i] : 0.f;
            f = r3::densify_flags(t, a, d, raw, opacity[i], radii);
        }
        out.flags[i] = f;
    }
    bool a, b, c;
    rows_of(f, in, a, b, c);
    __shared__ int s_count[kCounts][r3::kScanWaves];
    const bool flagged[kCounts] = {a, b, c, in && (f & r3::kFlagClone), in && (f & r3::kFlagSplit)};
    r3::block_count(flagged, s_count, out.counts + (long long)blockIdx.x * kCounts);
}

// One workgroup.  Round r takes the counts of plan workgroups r * kScanSpan + tid; the carry of the rounds before it lives in
// every thread's registers.
__global__ __launch_bounds__(kBlock) void scan_kernel(int P, long long nb, Plan p, int* __restrict__ totals)
{
    const int tid = threadIdx.x;
    __shared__ int s_wave[kCounts][r3::kScanWaves];
    int carry[kCounts] = {0, 0, 0, 0, 0};
    for (long long b0 = 0; b0 < nb; b0 += r3::kScanSpan) {
        const long long b = b0 + tid;
        int v[kCounts], inc[kCounts], excl[kCounts];
        r3::scan_round_publish(p.counts, b, nb, v, inc, s_wave);
        __syncthreads();
        r3::scan_round_combine(v, inc, s_wave, carry, excl);
#pragma unroll
        for (int k = 0; k < kSegCounts; k++)
            if (b < nb) p.offsets[b * kSegCounts + k] = excl[k];
        __syncthreads();   // s_wave is rewritten by the next round
    }
    if (tid == 0) {
        const int nA = carry[0], nB = carry[1], nC = carry[2], cloned = carry[3], split = carry[4];
        const int out_rows = nA + nB + 2 * nC;
        // the prune mask is taken over the set after clone and split: P - split + cloned + 2 split rows, out_rows survive
        const int pruned = P - split + cloned + r3::kSplitChildren * split - out_rows;
        const int t[R3DGS_DENSIFY_TOTALS] = {nA, nB, nC, nC, cloned, split, pruned, out_rows};
#pragma unroll
        for (int k = 0; k < R3DGS_DENSIFY_TOTALS; k++) {
            totals[k] = t[k];
            p.header[k] = t[k];
        }
        p.header[R3DGS_DENSIFY_TOTALS] = P;
    }
}

// The source Gaussian of every destination row: the lane's rank inside the workgroup plus the workgroup's first row of each
// segment, the scan's offsets.
__global__ __launch_bounds__(kBlock) void map_kernel(int P, Plan p)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < P;
    const uint8_t f = in ? p.flags[i] : 0;
    bool row[kSegCounts];
    rows_of(f, in, row[0], row[1], row[2]);
    __shared__ int s_count[kSegCounts][r3::kScanWaves];
    int rank[kSegCounts];
    r3::block_rank(row, s_count, rank);
    const int nA = p.header[0], nB = p.header[1], nC = p.header[2];
    const int first[kSegCounts] = {0, nA, nA + nB};
#pragma unroll
    for (int k = 0; k < kSegCounts; k++) {
        if (!row[k]) continue;
        const int r = rank[k] + p.offsets[(long long)blockIdx.x * kSegCounts + k];
        p.map[first[k] + r] = (int)i;
        if (k == 2) p.map[first[k] + nC + r] = (int)i;   // segment D: the second child, same rank
    }
}

struct Entry : r3::RowEntry {
    int dst_vec, src_vec;   // the base is 16-byte aligned
};
struct MoveTable {
    int n, P, nA, nB, nC, pad;
    const int* header;
    const int* map;
    const float *xyz, *scaling, *rotation, *noise;
    Entry e[kMaxTensors];
};
static_assert(sizeof(MoveTable) <= 3072, "the table travels as a by-value kernel argument");

// One word of a row of segment B (seg 1), C (2) or D (3) whose source Gaussian is `src`.
__device__ __forceinline__ uint32_t new_row_word(const MoveTable& t, const Entry& e, int seg, long long src, int w)
{
    if (e.kind == R3DGS_DENSIFY_ZERO_NEW) return 0u;
    if (seg >= 2 && e.kind == R3DGS_DENSIFY_XYZ) {
        const float* nz = t.noise + ((long long)(seg - 2) * t.P + src) * 3;
        const float rq[4] = {t.rotation[4 * src], t.rotation[4 * src + 1], t.rotation[4 * src + 2], t.rotation[4 * src + 3]};
        const float sc[3] = {r3::scale_act(t.scaling[3 * src]), r3::scale_act(t.scaling[3 * src + 1]),
                             r3::scale_act(t.scaling[3 * src + 2])};
        const float noise[3] = {nz[0], nz[1], nz[2]};
        return __float_as_uint(r3::child_xyz(w, rq, sc, noise, t.xyz[3 * src + w]));
    }
    if (seg >= 2 && e.kind == R3DGS_DENSIFY_SCALING)
        return __float_as_uint(r3::child_scaling(r3::scale_act(t.scaling[3 * src + w])));
    return e.src[src * e.W + w];
}

__global__ __launch_bounds__(kBlock) void move_kernel(const MoveTable t)
{
    // a plan made for other sizes than the caller claims: write nothing rather than follow a map that is not there
    if (t.header[0] != t.nA || t.header[1] != t.nB || t.header[2] != t.nC || t.header[R3DGS_DENSIFY_TOTALS] != t.P) return;
    const long long b = blockIdx.x;
    const Entry& e = t.e[r3::entry_of(t.e, t.n, b)];
    const int W = e.W;
    const long long block_first = (b - e.chunk_begin) * kChunkWords;   // wave-uniform: one 64-bit divide per workgroup
    const long long block_row = block_first / W;
    const uint32_t local = (uint32_t)(block_first - block_row * W) + kUnitWords * threadIdx.x;   // < W + kChunkWords
    long long row = block_row + local / (uint32_t)W;
    int w = (int)(local % (uint32_t)W);
    const long long first = block_first + kUnitWords * (long long)threadIdx.x;
    if (first >= e.words) return;
    const int nw = e.words - first < kUnitWords ? (int)(e.words - first) : kUnitWords;
    const long long endA = t.nA, endB = endA + t.nB, endC = endB + t.nC;
    auto seg_of = [&](long long r) { return r < endA ? 0 : r < endB ? 1 : r < endC ? 2 : 3; };

    if (e.dst_vec && e.src_vec && nw == kUnitWords && w + kUnitWords <= W) {   // the unit lies inside one row
        const int seg = seg_of(row);
        const bool copied = seg == 0 || e.kind == R3DGS_DENSIFY_COPY || (seg == 1 && e.kind != R3DGS_DENSIFY_ZERO_NEW);
        const long long so = (long long)t.map[row] * W + w;
        if (copied && (so & 3) == 0) {
            *reinterpret_cast<uint4*>(e.dst + first) = *reinterpret_cast<const uint4*>(e.src + so);
            return;
        }
    }
    uint32_t v[kUnitWords] = {0u, 0u, 0u, 0u};
    long long src = -1, src_row = -1;
    int seg = 0;
#pragma unroll
    for (int k = 0; k < kUnitWords; k++) {
        if (k < nw) {
            if (w == W) {
                w = 0;
                row++;
            }
            if (row != src_row) {
                src_row = row;
                src = t.map[row];
                seg = seg_of(row);
            }
            v[k] = seg == 0 ? e.src[src * W + w] : new_row_word(t, e, seg, src, w);
            w++;
        }
    }
    if (e.dst_vec && nw == kUnitWords) {
        *reinterpret_cast<uint4*>(e.dst + first) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kUnitWords; k++)
            if (k < nw) e.dst[first + k] = v[k];
    }
}

void check_plan_args(const char* what, int P, const char* workspace, const int* totals)
{
    if (P > kMaxP) throw r3::Error(std::string(what) + ": P exceeds 2^30");
    if (!workspace || !totals) throw r3::Error(std::string(what) + ": workspace or totals is NULL");
    if ((uintptr_t)workspace % 16) throw r3::Error(std::string(what) + ": workspace must be 16-byte aligned");
    if ((uintptr_t)totals % 4) throw r3::Error(std::string(what) + ": totals is not 4-byte aligned");
}

void finish_plan(int P, const Plan& plan, int* totals, hipStream_t s)
{
    const long long nb = plan_blocks(P);
    scan_kernel<<<1, kBlock, 0, s>>>(P, nb, plan, totals);
    r3::check_launch("densify scan", s, false);
    map_kernel<<<(unsigned)nb, kBlock, 0, s>>>(P, plan);
    r3::check_launch("densify map", s, false);
}

__global__ void zero_totals_kernel(int* totals)
{
    if (threadIdx.x < R3DGS_DENSIFY_TOTALS) totals[threadIdx.x] = 0;
}

}  // namespace

extern "C" {

size_t r3dgs_densify_workspace_bytes(int P)
{
    if (P <= 0 || P > kMaxP) return 0;
    return carve_plan(nullptr, P, nullptr);
}

int r3dgs_densify_plan(int P, int densify, const float* accum, const float* denom, const float* scaling, const float* opacity,
                       const float* max_radii2D, float max_grad, float dense_scale, float min_opacity, int screen,
                       float max_screen, float world_scale, char* workspace, int* totals, void* stream)
{
    return r3::guarded_call([&]() {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (densify && !(max_grad > 0.f))
            throw r3::Error("densify_plan: max_grad must be > 0 (the reference takes the split decision after the clones were "
                            "appended with a zero gradient: max_grad <= 0 would split the clones)");
        if (P <= 0) {
            if (!totals) throw r3::Error("densify_plan: totals is NULL");
            zero_totals_kernel<<<1, 64, 0, s>>>(totals);
            r3::check_launch("densify plan (empty)", s, false);
            return 0;
        }
        check_plan_args("densify_plan", P, workspace, totals);
        if (!scaling || !opacity) throw r3::Error("densify_plan: scaling or opacity is NULL");
        if (densify && (!accum || !denom)) throw r3::Error("densify_plan: xyz_gradient_accum or denom is NULL");
        if (!densify && screen && !max_radii2D) throw r3::Error("densify_plan: max_radii2D is NULL");
        r3::DensifyThresholds t;
        t.max_grad = max_grad;
        t.dense_scale = dense_scale;
        t.min_opacity = min_opacity;
        t.max_screen = max_screen;
        t.world_scale = world_scale;
        t.densify = densify ? 1 : 0;
        t.screen = screen ? 1 : 0;
        Plan plan;
        carve_plan(workspace, P, &plan);
        plan_kernel<false><<<(unsigned)plan_blocks(P), kBlock, 0, s>>>(P, t, accum, denom, scaling, opacity, max_radii2D, nullptr,
                                                                       plan);
        r3::check_launch("densify plan", s, false);
        finish_plan(P, plan, totals, s);
        return 0;
    });
}

int r3dgs_prune_plan(int P, const uint8_t* mask, char* workspace, int* totals, void* stream)
{
    return r3::guarded_call([&]() {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (P <= 0) {
            if (!totals) throw r3::Error("prune_plan: totals is NULL");
            zero_totals_kernel<<<1, 64, 0, s>>>(totals);
            r3::check_launch("prune plan (empty)", s, false);
            return 0;
        }
        check_plan_args("prune_plan", P, workspace, totals);
        if (!mask) throw r3::Error("prune_plan: mask is NULL");
        Plan plan;
        carve_plan(workspace, P, &plan);
        plan_kernel<true><<<(unsigned)plan_blocks(P), kBlock, 0, s>>>(P, r3::DensifyThresholds{}, nullptr, nullptr, nullptr, nullptr,
                                                                      nullptr, mask, plan);
        r3::check_launch("prune plan", s, false);
        finish_plan(P, plan, totals, s);
        return 0;
    });
}

int r3dgs_densify_move(int P, int nA, int nB, int nC, int n, const r3dgs_densify_tensor* tensors, const float* xyz,
                       const float* scaling, const float* rotation, const float* noise, const char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        if (P < 0 || P > kMaxP) throw r3::Error("densify_move: P out of range");
        if (nA < 0 || nB < 0 || nC < 0 || nA > P || nB > P || nC > P || (long long)nA + nB + 2LL * nC > 2LL * P)
            throw r3::Error("densify_move: segment sizes do not fit P source Gaussians");
        if (n < 0 || n > kMaxTensors) throw r3::Error("densify_move: more than R3DGS_DENSIFY_MAX_TENSORS tensors");
        const long long rows = (long long)nA + nB + 2LL * nC;
        if (rows == 0 || n == 0) return 0;
        if (!tensors) throw r3::Error("densify_move: tensors is NULL");
        if (!workspace || (uintptr_t)workspace % 16) throw r3::Error("densify_move: workspace is NULL or not 16-byte aligned");
        if (nC > 0 && (!xyz || !scaling || !rotation || !noise))
            throw r3::Error("densify_move: split rows need xyz, scaling, rotation and noise");
        Plan plan;
        carve_plan(const_cast<char*>(workspace), P, &plan);
        MoveTable t{};
        t.P = P;
        t.nA = nA;
        t.nB = nB;
        t.nC = nC;
        t.header = plan.header;
        t.map = plan.map;
        t.xyz = xyz;
        t.scaling = scaling;
        t.rotation = rotation;
        t.noise = noise;
        const long long chunks = r3::fill_entries(
            "densify_move", tensors, n, rows, kChunkWords, R3DGS_DENSIFY_SCALING,
            [](int kind, int row_words) {
                const bool child = kind == R3DGS_DENSIFY_XYZ || kind == R3DGS_DENSIFY_SCALING;
                return child && row_words != 3 ? ": xyz and scaling rows have 3 words" : nullptr;
            },
            nullptr, t.e, t.n);
        for (int i = 0; i < t.n; i++) {
            t.e[i].dst_vec = (uintptr_t)t.e[i].dst % 16 == 0;
            t.e[i].src_vec = (uintptr_t)t.e[i].src % 16 == 0;
        }
        if (chunks == 0) return 0;
        hipStream_t s = static_cast<hipStream_t>(stream);
        move_kernel<<<(unsigned)chunks, kBlock, 0, s>>>(t);
        r3::check_launch("densify move", s, false);
        return 0;
    });
}

}  // extern "C"
