// mcmc.hip -- the fixed-budget densification strategy of include/r3dgs_mcmc.h (3DGS-MCMC): the per-iteration noise term, the
// plan that relocation and growth share, and the move of the model's tensors.  Per-Gaussian arithmetic: mcmc_math.h.
//
// wave64, 256-thread workgroups, no float atomics, no host wait, no allocation.
//   noise   one launch, one lane per Gaussian: the 56 bytes a Gaussian reads are loaded first (12-byte rows as one three-word
//           load each, the quaternion as one 16-byte load), then the arithmetic, then one 12-byte store.  The covariance is never
//           formed: v = R^T n, v_j *= s_j^2, R v.
//   plan    weights  one lane per Gaussian: its weight (fp32 sigmoid, 0 for a dead row), ratio = 1, and per workgroup the
//                    double sum of the weights (a fixed tree) and the counts of dead rows and of rows of positive weight.
//           scan     ONE workgroup walks the per-workgroup sums and counts in rounds of kScanSpan (block_scan.h) and
//                    writes the header: total weight, dead, positive, draws, the no-op flag.
//           cdf      one lane per Gaussian again: cdf = workgroup offset + the same tree's inclusive value; a row of positive
//                    weight writes (cdf, index) at its rank among the positive rows, a dead row writes its index into slots.
//                    The draw searches the COMPACTED cdf: whatever it returns is a row of positive weight by construction,
//                    for any u and however the double sums round.
//           draw     one lane per draw: binary search, sampled[k], integer atomic ratio[j] += 1 (order-independent).
//           finish   one lane per Gaussian: clamps ratio to 51, counts the distinct and the clamped sources.
//   move    values   one lane per Gaussian: a drawn source's new raw opacity and scaling, into the workspace -- so that no
//                    row of the in-place relocation is read while it is half-written.
//           relocate / grow   one thread per 4-byte word of every tensor of the table.
// The workgroup scans, counts and ranks are block_scan.h's; the workspace carver and the tensor table row_table.h's.
#include "../../include/r3dgs_mcmc.h"

#include "block_scan.h"
#include "mcmc_math.h"
#include "row_table.h"

namespace {

constexpr int kBlock = r3::kScanBlock;
constexpr int kWaves = r3::kScanWaves;
constexpr int kMaxTensors = R3DGS_MCMC_MAX_TENSORS;
constexpr long long kMaxP = r3::kMaxP;
constexpr int kValWords = 4;        // new raw opacity, three new raw scales
using r3::plan_blocks;
static_assert(kBlock == r3::kPlanBlock && R3DGS_MCMC_COPY == 0, "row_table.h's grid and kind range");

__constant__ r3::McmcBinom kBinom = r3::make_mcmc_binom();

struct Header {
    double total;   // cdf[P-1]
    int dead, pos, draws, noop, P, mode;
    int pad[8];
};
static_assert(sizeof(Header) == 64, "the header is 64 bytes");

struct Plan {
    Header* header;
    int* counts;     // [nb][2] dead rows, rows of positive weight
    int* offs;       // [nb][2] their exclusive scans
    double* sums;    // [nb] weight of the workgroup
    double* soff;    // [nb] exclusive scan
    double* cdf;     // [pos] cdf of the rows of positive weight, in index order
    int* idx;        // [pos] their indices
    float* vals;     // [P][kValWords] new raw opacity and scaling of the drawn sources (move)
};
// The layout of the workspace; with ws == NULL only its size.
inline size_t carve_plan(char* ws, long long P, Plan* p)
{
    const size_t nb = (size_t)plan_blocks(P);
    r3::Carver16 c{ws};
    Plan q;
    q.header = c.take<Header>(1);
    q.sums = c.take<double>(nb);
    q.soff = c.take<double>(nb);
    q.cdf = c.take<double>((size_t)P);
    q.counts = c.take<int>(nb * 2);
    q.offs = c.take<int>(nb * 2);
    q.idx = c.take<int>((size_t)P);
    q.vals = c.take<float>((size_t)P * kValWords);
    if (p) *p = q;
    return c.used();
}

// ---- noise ----------------------------------------------------------------------------------------------------------------

struct __attribute__((packed, aligned(4))) Row3 {
    float v[3];
};

__global__ __launch_bounds__(kBlock) void noise_kernel(int P, float* __restrict__ xyz, const float* __restrict__ opacity,
                                                       const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                       const float* __restrict__ noise, float scale)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P) return;
    // every load of the lane, before anything waits on one of them
    const float4 q4 = reinterpret_cast<const float4*>(rotation)[i];
    const Row3 n = reinterpret_cast<const Row3*>(noise)[i];
    const Row3 s = reinterpret_cast<const Row3*>(scaling)[i];
    const Row3 x = reinterpret_cast<const Row3*>(xyz)[i];
    const float o = opacity[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    float d[3];
    r3::mcmc_noise_delta(q, s.v, o, n.v, scale, d);
    Row3 out;
#pragma unroll
    for (int k = 0; k < 3; k++) out.v[k] = r3::mcmc_displace(x.v[k], d[k]);
    reinterpret_cast<Row3*>(xyz)[i] = out;
}

// ---- plan -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void weights_kernel(int P, const float* __restrict__ opacity, float min_opacity, int relocate,
                                                         int* __restrict__ ratio, Plan out)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < P;
    bool dead = false;
    const float w = in ? r3::mcmc_weight(opacity[i], min_opacity, relocate, dead) : 0.f;
    if (in) ratio[i] = 1;
    __shared__ double s_wave[kWaves];
    __shared__ int s_count[2][kWaves];
    double total;
    r3::block_scan((double)w, s_wave, total);
    const bool flag[2] = {dead, w > 0.f};
    r3::block_count(flag, s_count, out.counts + (long long)blockIdx.x * 2);
    if (threadIdx.x == 0) out.sums[blockIdx.x] = total;
}

// One workgroup.  Round r takes plan workgroups r * kScanSpan + tid; the carries live in every thread's registers.
__global__ __launch_bounds__(kBlock) void scan_kernel(int P, int mode, int n_draws, long long nb, Plan p, int* __restrict__ totals)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_int[2][kWaves];
    __shared__ double s_wave[kWaves];
    int carry[2] = {0, 0};
    double wcarry = 0.0;
    for (long long b0 = 0; b0 < nb; b0 += r3::kScanSpan) {
        const long long b = b0 + tid;
        int v[2], inc[2], off[2];
        r3::scan_round_publish(p.counts, b, nb, v, inc, s_int);
        const double wv = b < nb ? p.sums[b] : 0.0;
        double wall;
        const double winc = r3::block_scan(wv, s_wave, wall);   // its barrier also publishes s_int
        r3::scan_round_combine(v, inc, s_int, carry, off);
        if (b < nb) {
            p.offs[b * 2] = off[0];
            p.offs[b * 2 + 1] = off[1];
        }
        // the offset of workgroup b: everything before the round, plus the round's inclusive value of workgroup b - 1 (the
        // exclusive value is never formed by a subtraction)
        const double wprev = __shfl_up(winc, 1);
        __shared__ double s_last[kWaves];
        if (lane == 63) s_last[wave] = winc;
        __syncthreads();
        const double excl = tid == 0 ? 0.0 : (lane == 0 ? s_last[wave - 1] : wprev);
        if (b < nb) p.soff[b] = wcarry + excl;
        wcarry += wall;
        __syncthreads();   // the LDS is rewritten by the next round
    }
    if (tid == 0) {
        const int dead = carry[0], pos = carry[1];
        const int want = mode == R3DGS_MCMC_RELOCATE ? dead : n_draws;
        const int noop = pos == 0 ? 1 : (want == 0 ? 2 : 0);
        const int draws = noop ? 0 : want;
        Header h{};
        h.total = wcarry;
        h.dead = dead;
        h.pos = pos;
        h.draws = draws;
        h.noop = noop;
        h.P = P;
        h.mode = mode;
        *p.header = h;
        const int t[R3DGS_MCMC_TOTALS] = {dead, draws, 0, 0, noop, pos, 0, 0};
#pragma unroll
        for (int k = 0; k < R3DGS_MCMC_TOTALS; k++) totals[k] = t[k];
    }
}

__global__ __launch_bounds__(kBlock) void cdf_kernel(int P, const float* __restrict__ opacity, float min_opacity, int relocate,
                                                     int* __restrict__ slots, Plan p)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < P;
    bool dead = false;
    const float w = in ? r3::mcmc_weight(opacity[i], min_opacity, relocate, dead) : 0.f;
    __shared__ double s_wave[kWaves];
    __shared__ int s_count[2][kWaves];
    double total;
    const double inc = r3::block_scan((double)w, s_wave, total);
    const bool flag[2] = {dead, w > 0.f};
    int rank[2];
    r3::block_rank(flag, s_count, rank);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!flag[k]) continue;
        const int r = rank[k] + p.offs[(long long)blockIdx.x * 2 + k];
        if (r < 0 || r >= P) continue;   // cannot happen with the scan's own offsets
        if (k == 0) {
            if (slots) slots[r] = (int)i;
        } else {
            p.cdf[r] = p.soff[blockIdx.x] + inc;
            p.idx[r] = (int)i;
        }
    }
}

__global__ __launch_bounds__(kBlock) void draw_kernel(int P, int n_max, const float* __restrict__ uniforms,
                                                      int* __restrict__ sampled, int* __restrict__ ratio, Plan p)
{
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_max) return;
    const Header h = *p.header;
    if (h.noop) {   // GROW with nothing to draw from: the grown rows become plain copies
        if (h.mode == R3DGS_MCMC_GROW && h.noop == 1) sampled[k] = (int)(k % P);
        return;
    }
    if (k >= h.draws) return;
    const int m = r3::mcmc_search(p.cdf, h.pos, r3::mcmc_target(uniforms[k], h.total));
    const int j = p.idx[m];
    sampled[k] = j;
    if (j >= 0 && j < P) atomicAdd(&ratio[j], 1);
}

__global__ __launch_bounds__(kBlock) void finish_kernel(int P, int* __restrict__ ratio, int* __restrict__ totals)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const long long i = (long long)blockIdx.x * kBlock + tid;
    const int r = i < P ? ratio[i] : 1;
    if (r > r3::kMcmcMaxRatio) ratio[i] = r3::mcmc_ratio_clamp(r);
    const int distinct = (int)__popcll(__ballot(r > 1)), clamped = (int)__popcll(__ballot(r > r3::kMcmcMaxRatio));
    if (lane == 0) {   // integer atomics: the sums do not depend on the order
        if (distinct) atomicAdd(&totals[2], distinct);
        if (clamped) atomicAdd(&totals[3], clamped);
    }
}

__global__ void empty_totals_kernel(int* totals)
{
    if (threadIdx.x < R3DGS_MCMC_TOTALS) totals[threadIdx.x] = threadIdx.x == 4 ? 1 : 0;
}

// ---- move -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void values_kernel(int P, const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                        const int* __restrict__ ratio, float min_opacity, float* __restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)P) return;
    const int N = r3::mcmc_ratio_clamp(ratio[i]);
    if (N < 2) return;
    const float raw[3] = {scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]};
    float no, ns[3];
    r3::mcmc_relocate(opacity[i], raw, N, min_opacity, kBinom, no, ns);
    vals[kValWords * i] = no;
    vals[kValWords * i + 1] = ns[0];
    vals[kValWords * i + 2] = ns[1];
    vals[kValWords * i + 3] = ns[2];
}

using Entry = r3::RowEntry;   // words: P rows (RELOCATE) or P + n_new rows (GROW)
struct MoveTable {
    int n, P, n_new, zero_relocated;
    const int *sampled, *slots, *ratio, *totals;
    const uint32_t* vals;
    Entry e[kMaxTensors];
};
static_assert(sizeof(MoveTable) <= 3072, "the table travels as a by-value kernel argument");

// The word (row s, w) of tensor e as a relocated / new row copies it: the updated value of a drawn source.
__device__ __forceinline__ uint32_t updated_word(const MoveTable& t, const Entry& e, long long s, int w, bool drawn)
{
    if (drawn && e.kind == R3DGS_MCMC_OPACITY) return t.vals[kValWords * s];
    if (drawn && e.kind == R3DGS_MCMC_SCALING) return t.vals[kValWords * s + 1 + w];
    return e.src[s * e.W + w];
}

__device__ __forceinline__ bool locate(const MoveTable& t, int& ei, long long& g)
{
    const long long b = blockIdx.x;
    ei = r3::entry_of(t.e, t.n, b);
    g = (b - t.e[ei].chunk_begin) * kBlock + threadIdx.x;
    return g < t.e[ei].words;
}

// In place.  Thread (row r, word w) of a tensor plays two parts: the row r itself, if it is a drawn source; and draw r, if
// there is one -- the dead row slots[r] becomes a copy of the updated source sampled[r].  Sources are alive and destinations
// dead, so no word is written twice, and what a copy reads is either a word nobody writes or the workspace.
__global__ __launch_bounds__(kBlock) void relocate_kernel(const MoveTable t)
{
    int ei;
    long long g;
    if (!locate(t, ei, g)) return;
    const Entry& e = t.e[ei];
    const long long r = g / e.W;
    const int w = (int)(g - r * e.W);
    if (t.ratio[r] >= 2) {
        if (e.kind == R3DGS_MCMC_MOMENT)
            e.dst[g] = 0u;
        else if (e.kind != R3DGS_MCMC_COPY)
            e.dst[g] = updated_word(t, e, r, w, true);
    }
    if (r < t.totals[1]) {
        const long long d = t.slots[r], s = t.sampled[r];
        if (d < 0 || d >= t.P || s < 0 || s >= t.P) return;
        if (e.kind == R3DGS_MCMC_MOMENT) {
            if (t.zero_relocated) e.dst[d * e.W + w] = 0u;
        } else {
            e.dst[d * e.W + w] = updated_word(t, e, s, w, true);
        }
    }
}

__global__ __launch_bounds__(kBlock) void grow_kernel(const MoveTable t)
{
    int ei;
    long long g;
    if (!locate(t, ei, g)) return;
    const Entry& e = t.e[ei];
    const long long r = g / e.W;
    const int w = (int)(g - r * e.W);
    long long s = r;
    const bool is_new = r >= t.P;
    if (is_new) {
        s = t.sampled[r - t.P];
        if (s < 0 || s >= t.P) {
            e.dst[g] = 0u;
            return;
        }
    }
    e.dst[g] = (is_new && e.kind == R3DGS_MCMC_MOMENT) ? 0u : updated_word(t, e, s, w, t.ratio[s] >= 2);
}

}  // namespace

extern "C" {

size_t r3dgs_mcmc_workspace_bytes(int P, int n_draws)
{
    if (P <= 0 || P > kMaxP || n_draws < 0) return 0;
    return carve_plan(nullptr, P, nullptr);
}

int r3dgs_mcmc_noise(int P, float* xyz, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
                     const float* noise, float scale, void* stream)
{
    return r3::guarded_call([&]() {
        if (P <= 0) return 0;
        if (P > kMaxP) throw r3::Error("mcmc_noise: P exceeds 2^30");
        if (!xyz || !opacity_raw || !scaling_raw || !rotation_raw || !noise) throw r3::Error("mcmc_noise: a tensor is NULL");
        if ((uintptr_t)xyz % 4 || (uintptr_t)opacity_raw % 4 || (uintptr_t)scaling_raw % 4 || (uintptr_t)noise % 4)
            throw r3::Error("mcmc_noise: a tensor is not 4-byte aligned");
        if ((uintptr_t)rotation_raw % 16) throw r3::Error("mcmc_noise: rotation_raw must be 16-byte aligned");
        hipStream_t s = static_cast<hipStream_t>(stream);
        noise_kernel<<<(unsigned)plan_blocks(P), kBlock, 0, s>>>(P, xyz, opacity_raw, scaling_raw, rotation_raw, noise, scale);
        r3::check_launch("mcmc noise", s, false);
        return 0;
    });
}

int r3dgs_mcmc_plan(int P, const float* opacity_raw, float min_opacity, int mode, int n_draws, const float* uniforms,
                    int* sampled, int* slots, int* ratio, int* totals, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (mode != R3DGS_MCMC_RELOCATE && mode != R3DGS_MCMC_GROW) throw r3::Error("mcmc_plan: unknown mode");
        if (!totals || (uintptr_t)totals % 4) throw r3::Error("mcmc_plan: totals is NULL or not 4-byte aligned");
        if (P <= 0) {
            empty_totals_kernel<<<1, 64, 0, s>>>(totals);
            r3::check_launch("mcmc plan (empty)", s, false);
            return 0;
        }
        if (P > kMaxP) throw r3::Error("mcmc_plan: P exceeds 2^30");
        const bool relocate = mode == R3DGS_MCMC_RELOCATE;
        if (relocate) n_draws = P;   // at most: the number of dead rows is counted on the device
        if (n_draws < 0 || n_draws > kMaxP) throw r3::Error("mcmc_plan: n_draws out of range");
        if (!workspace || (uintptr_t)workspace % 16) throw r3::Error("mcmc_plan: workspace is NULL or not 16-byte aligned");
        if (!opacity_raw || !ratio) throw r3::Error("mcmc_plan: opacity_raw or ratio is NULL");
        if (relocate && !slots) throw r3::Error("mcmc_plan: slots is NULL");
        if (n_draws > 0 && (!uniforms || !sampled)) throw r3::Error("mcmc_plan: uniforms or sampled is NULL");
        Plan plan;
        carve_plan(workspace, P, &plan);
        const long long nb = plan_blocks(P);
        weights_kernel<<<(unsigned)nb, kBlock, 0, s>>>(P, opacity_raw, min_opacity, relocate ? 1 : 0, ratio, plan);
        r3::check_launch("mcmc weights", s, false);
        scan_kernel<<<1, kBlock, 0, s>>>(P, mode, relocate ? 0 : n_draws, nb, plan, totals);
        r3::check_launch("mcmc scan", s, false);
        cdf_kernel<<<(unsigned)nb, kBlock, 0, s>>>(P, opacity_raw, min_opacity, relocate ? 1 : 0, relocate ? slots : nullptr, plan);
        r3::check_launch("mcmc cdf", s, false);
        if (n_draws > 0) {
            draw_kernel<<<(unsigned)plan_blocks(n_draws), kBlock, 0, s>>>(P, n_draws, uniforms, sampled, ratio, plan);
            r3::check_launch("mcmc draw", s, false);
        }
        finish_kernel<<<(unsigned)nb, kBlock, 0, s>>>(P, ratio, totals);
        r3::check_launch("mcmc finish", s, false);
        return 0;
    });
}

int r3dgs_mcmc_move(int P, int mode, int n_new, int zero_relocated, float min_opacity, int n, const r3dgs_mcmc_tensor* tensors,
                    const float* opacity_raw, const float* scaling_raw, const int* sampled, const int* slots, const int* ratio,
                    const int* totals, char* workspace, void* stream)
{
    return r3::guarded_call([&]() {
        if (mode != R3DGS_MCMC_RELOCATE && mode != R3DGS_MCMC_GROW) throw r3::Error("mcmc_move: unknown mode");
        const bool relocate = mode == R3DGS_MCMC_RELOCATE;
        if (P < 0 || P > kMaxP) throw r3::Error("mcmc_move: P out of range");
        if (n_new < 0 || (long long)P + n_new > kMaxP || (relocate && n_new != 0) || (P == 0 && n_new != 0))
            throw r3::Error("mcmc_move: n_new does not fit the mode and P");
        if (n < 0 || n > kMaxTensors) throw r3::Error("mcmc_move: more than R3DGS_MCMC_MAX_TENSORS tensors");
        if (P == 0 || n == 0 || (!relocate && n_new == 0)) return 0;
        if (!tensors) throw r3::Error("mcmc_move: tensors is NULL");
        if (!workspace || (uintptr_t)workspace % 16) throw r3::Error("mcmc_move: workspace is NULL or not 16-byte aligned");
        if (!opacity_raw || !scaling_raw || !sampled || !ratio || !totals || (relocate && !slots))
            throw r3::Error("mcmc_move: opacity_raw, scaling_raw, sampled, slots, ratio or totals is NULL");
        Plan plan;
        carve_plan(workspace, P, &plan);
        MoveTable t{};
        t.P = P;
        t.n_new = n_new;
        t.zero_relocated = zero_relocated ? 1 : 0;
        t.sampled = sampled;
        t.slots = slots;
        t.ratio = ratio;
        t.totals = totals;
        t.vals = reinterpret_cast<const uint32_t*>(plan.vals);
        const long long rows = (long long)P + n_new;
        const long long chunks = r3::fill_entries(
            "mcmc_move", tensors, n, rows, kBlock, R3DGS_MCMC_SCALING,
            [](int kind, int row_words) -> const char* {
                if (kind == R3DGS_MCMC_OPACITY && row_words != 1) return ": opacity rows have 1 word";
                return kind == R3DGS_MCMC_SCALING && row_words != 3 ? ": scaling rows have 3 words" : nullptr;
            },
            [relocate](const void* src, const void* dst) -> const char* {
                if (relocate && src != dst) return ": relocation is in place, src must equal dst";
                return !relocate && src == dst ? ": growth writes new tensors, src must differ from dst" : nullptr;
            },
            t.e, t.n);
        hipStream_t s = static_cast<hipStream_t>(stream);
        values_kernel<<<(unsigned)plan_blocks(P), kBlock, 0, s>>>(P, opacity_raw, scaling_raw, ratio, min_opacity, plan.vals);
        r3::check_launch("mcmc values", s, false);
        if (chunks == 0) return 0;
        if (relocate)
            relocate_kernel<<<(unsigned)chunks, kBlock, 0, s>>>(t);
        else
            grow_kernel<<<(unsigned)chunks, kBlock, 0, s>>>(t);
        r3::check_launch("mcmc move", s, false);
        return 0;
    });
}

}  // extern "C"
