// pass_driver.hip -- orchestration of one forward / backward pass behind the extern "C" boundary (capi.hip, through
// pass_driver.h); replaces CudaRasterizer::Rasterizer::{forward, inferenceForward, backward}
// (cuda_rasterizer/rasterizer_impl.cu:206-355, :359-504, :508-630 of the reference's diff-gaussian-rasterization).
// Also the library's state: the toggles, the stage profiler, the pass tickets with the host-mapped PassInfo ring, and the
// reservation advice (reserve_advice.h) wrapped around that ring.
// How the work is issued (results are the same as the reference's):
//   * The reference sizes its binning buffer from a blocking read-back of num_rendered in the middle of every forward
//     (rasterizer_impl.cu:441-450).  Here the hot path (r3dgs_forward_reserved) takes a pair RESERVATION instead:
//     the caller allocates the binning blob for `reserve` pairs up front, every kernel reads the actual count from
//     the device header, and the host never waits.  r3dgs_reserve_hint() proposes the reservation from the
//     num_rendered of earlier passes (published by the passes themselves in host-mapped memory, harvested lazily).
//     r3dgs_forward keeps the reference's exact-size contract (allocator callbacks, returns num_rendered): it waits
//     for that one number by polling host memory -- no HIP call, bounded by a deadline.
//   * All kernels of a pass read their arguments from one device-resident block (common.h), so the launch chain of
//     a shape never changes: it is captured once into a hipGraph and replayed with ONE hipGraphLaunch per pass
//     (+ one hipGraphExecKernelNodeSetParams that carries the new block).  Measured on the MI355X box
//     (tools/launch_bench*.hip): 20 direct launches cost 54 us of host time idle and 0.3-2.3 ms on a loaded /
//     CPU-throttled host, one graph launch 6-10 us either way; a graph with a side-stream branch costs as much as
//     direct launches, so the chain is linear.
//   * no per-call hipMalloc/hipFree: all scratch lives in the three caller blobs;
//   * `debug` and the per-stage timers issue the same chain with direct launches and synchronise / record events
//     between stages (the reference's CHECK_CUDA).
#include <time.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <unordered_map>
#include <vector>

#include "pass_driver.h"
#include "reserve_advice.h"
#include "unit_order.h"

namespace r3 {
int env_int(const char* env, int dflt, int lo, int hi)
{
    const char* v = getenv(env);
    if (!v) return dflt;
    const int p = atoi(v);
    return (p >= lo && p <= hi) ? p : dflt;
}
bool keep_quad_masks()   // R3DGS_KEEP_QUAD_MASKS=0: the backward repeats the forward's region pre-test (A/B runs)
{
    static const bool keep = env_int("R3DGS_KEEP_QUAD_MASKS", 1, 0, 1) != 0;
    return keep;
}
int bwd_segment_log2()
{
    static const int v = env_int("R3DGS_BWD_SEG_LEN", 128, 128, 256) == 256 ? 8 : 7;
    return v;
}
int bwd_segment_factor_pct()
{
    static const int v = env_int("R3DGS_BWD_SEG_FACTOR", 75, 10, 100000);
    return v;
}
int depth_bucket_load()
{
    static const int load = env_int("R3DGS_DEPTH_BUCKET_LOAD", 128, 32, 2048);   // 64 / 128 / 256 / 512 measured: 0.106 / 0.084 / 0.099 / 0.139 ms
    return load;
}

// Opacity-aware tile rects (gauss_math.h tighten_rect) are the default; R3DGS_TIGHT_RECT=0 / r3dgs_set_tight_rects(0)
// bins into the reference's 3-sigma squares (identical lists to the reference's: the bit-exact binning tests).
Toggle g_tight_rects{"R3DGS_TIGHT_RECT"};
// The backward blend starts its tiles heaviest first (unit_order.hip); R3DGS_TILE_ORDER=0 /
// r3dgs_set_tile_order(0): row-major bands, one per XCD, as the forward (A/B runs, the bit-identity test).
Toggle g_tile_order{"R3DGS_TILE_ORDER"};
// Long tile lists are walked by several workgroups of the backward blend, from checkpoints the forward blend leaves
// (common.h, blend.hip); R3DGS_BWD_SEG=0 / r3dgs_set_bwd_segments(0): one workgroup per tile whatever its list
// (A/B runs, the bit-identity tests of the launch order).
Toggle g_bwd_segments{"R3DGS_BWD_SEG"};
// Without a sparsity term the backward takes the SH direction derivatives the forward left (GeomState::sh_ddir) instead of
// reading every SH row again; R3DGS_SH_CACHE=0 / r3dgs_set_sh_cache(0): it reads the rows (A/B runs, the bit-identity test).
Toggle g_sh_cache{"R3DGS_SH_CACHE"};
// The per-Gaussian backward evaluates the covariance chain (backward.cu:228-306, 311-374) in double and rounds once
// (gauss_math.h); R3DGS_F64_CHAIN=0 / r3dgs_set_f64_chain(0): the reference's fp32 arithmetic (A/B runs).
Toggle g_f64_chain{"R3DGS_F64_CHAIN"};

size_t cached_depth_temp(size_t P)
{
    static std::mutex mu;
    static std::unordered_map<size_t, size_t> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(P);
    if (it != cache.end()) return it->second;
    size_t b = depth_sort_temp_bytes(P);
    cache[P] = b;
    return b;
}

size_t geometry_blob_bytes(size_t P, size_t depth_temp, bool lean)
{
    const GeomState g = GeomState::carve(nullptr, P, depth_temp);
    return (size_t)reinterpret_cast<uintptr_t>(lean ? g.lean_end : g.end) + kAlign;
}
}  // namespace r3

namespace {

using namespace r3;

thread_local int g_last_forward_pairs = 0;   // r3dgs_forward_pairs()
thread_local int g_next_forward_trains = 1;  // r3dgs_forward_hint(): holds for this thread's forwards until set again

int tight_rects() { return g_tight_rects.get(); }
int heaviest_tiles_first() { return g_tile_order.get(); }
int bwd_segments() { return g_bwd_segments.get(); }
int sh_derivative_cache() { return g_sh_cache.get(); }
int f64_chain() { return g_f64_chain.get(); }

bool env_is(const char* name, const char* value)
{
    const char* v = getenv(name);
    return v && std::string(v) == value;
}

// ---- the argument-block writers ------------------------------------------------------------------------------------
// The block travels as the kernel's by-value argument (so a replayed graph gets the new block with one
// hipGraphExecKernelNodeSetParams and nothing the host writes later can race with a queued launch) and is copied
// word-wise straight out of the kernarg segment: taking the parameter's address would first spill it to scratch.
template <class Block>
__global__ __launch_bounds__(256) void write_args_kernel(Block* dst, Block v)
{
    static_assert(alignof(Block) == 8 && sizeof(Block) % 4 == 0, "kernarg layout: [dst (8 B)][block]");
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const uint32_t __attribute__((address_space(4))) * KernargWords;
    KernargWords s = (KernargWords)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(Block*) / 4;
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (uint32_t k = threadIdx.x; k < sizeof(Block) / 4; k += 256) d[k] = s[k];
#endif
    (void)v;
}

// ---- optional per-stage timing with HIP events on the caller's stream (r3dgs_profile_*) ----------
struct Profiler {
    std::mutex mu;
    std::atomic<unsigned> mask{0};   // bit (stage): record an event pair around that stage
    std::vector<std::pair<hipEvent_t, hipEvent_t>> used[kNumStages];
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        R3_HIP(hipEventCreate(&e));
        return e;
    }
} g_prof;
constexpr unsigned kFwdStages = (1u << kPre) | (1u << kDepthSort) | (1u << kBinning) | (1u << kBlendFwd) | (1u << kColor);
constexpr unsigned kBwdStages = (1u << kBlendBwd) | (1u << kPreBwd) | (1u << kBlendBwdKernel);

struct StageRun {   // direct-issue mode: events and / or debug synchronisation around each stage
    bool debug;
    hipEvent_t a[kNumStages] = {};
    void begin(int stage, hipStream_t s)
    {
        if (!((g_prof.mask.load() >> stage) & 1u)) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        a[stage] = g_prof.get();
        R3_HIP(hipEventRecord(a[stage], s));
    }
    void end(int stage, const char* what, hipStream_t s)
    {
        if (a[stage]) {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            hipEvent_t b = g_prof.get();
            R3_HIP(hipEventRecord(b, s));
            g_prof.used[stage].push_back({a[stage], b});
            a[stage] = nullptr;
        }
        check_launch(what, s, debug);
    }
};

// ---- pass tickets (reserve_advice.h) and the host-mapped PassInfo ring ----------------------------------------------
struct InfoRing {
    PassInfo* host = nullptr;
    PassInfo* dev = nullptr;
};
std::mutex g_ring_mu;
std::unordered_map<int, InfoRing> g_rings;
std::atomic<uint64_t> g_next_ticket{1};

InfoRing& info_ring(int dev)
{
    std::lock_guard<std::mutex> lk(g_ring_mu);
    InfoRing& r = g_rings[dev];
    if (!r.host) {
        R3_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.host), sizeof(PassInfo) * kInfoRing,
                             hipHostMallocMapped | hipHostMallocCoherent));
        memset(r.host, 0, sizeof(PassInfo) * kInfoRing);
        R3_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&r.dev), r.host, 0));
    }
    return r;
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Wait until the pass has published its header (num_rendered, visible).  Plain loads of host memory: a spin of up to
// ~100 us (R3DGS_SPIN_US), then sleeps -- a spinning thread burns CPU quota that a containerised trainer may not have,
// but a sleep of "5 us" returns after 50-60 (timer slack), which a 10 k-Gaussian scene whose whole step takes 0.15 ms of
// GPU time pays on every forward (4000 instead of 5600 it/s) -- and a deadline (R3DGS_SYNC_TIMEOUT_MS, default 30 s) that
// turns a hung GPU into an error instead of a hung host.
const volatile PassInfo* wait_info(uint64_t ticket)
{
    static const int timeout_ms = env_int("R3DGS_SYNC_TIMEOUT_MS", 30000, 1, 3600000);
    static const int spin_us = env_int("R3DGS_SPIN_US", 100, 0, 1000000);
    const volatile PassInfo* info = info_ring(ticket_device(ticket)).host + ticket_number(ticket) % kInfoRing;
    const uint32_t seq = (uint32_t)ticket_number(ticket);
    const double t0 = now_ms();
    for (int spins = 0;; spins++) {
        if (info->seq == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return info;
        }
        if ((spins & 63) != 63) continue;   // look at the clock every 64 polls
        const double waited = now_ms() - t0;
        if (waited * 1000.0 < (double)spin_us) continue;
        if (waited > timeout_ms)
            throw Error("timed out after " + std::to_string(timeout_ms) + " ms waiting for num_rendered of pass " +
                        std::to_string(ticket_number(ticket)) + " (GPU hung or stream never ran?)");
        timespec ts = {0, waited < 2.0 ? 5000 : 50000};
        nanosleep(&ts, nullptr);
    }
}

// ---- the reservation advice (reserve_advice.h) over the ring ----------------------------------------------------------
Advisor g_adv;

// What a harvest asks of a pass: has it published its header -- and, if its depth scan stamps one, the overflow hint of
// the bucketed depth sort, which comes from a later kernel than the header and carries its own stamp?
bool pass_published(const Pending& p, uint32_t* pairs, uint32_t* sort_overflow)
{
    const uint64_t n = ticket_number(p.ticket);
    const volatile PassInfo* info = info_ring(p.dev).host + n % kInfoRing;
    if (info->seq != (uint32_t)n || (p.sort_stamp && info->sort_seq != (uint32_t)n)) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    *pairs = info->pairs;
    *sort_overflow = p.sort_stamp ? info->sort_overflow : 0u;
    return true;
}

int current_device()
{
    int dev = 0;
    R3_HIP(hipGetDevice(&dev));
    return dev;
}

// ---- launch contexts: device argument blocks and captured graphs ---------------------------------------------------
struct CtxKey {
    int dev, kind;   // kind 0: forward, 1: backward
    hipStream_t stream;
    int P, M, W, H;
    uint32_t reserve, flags;
    bool operator<(const CtxKey& o) const
    {
        return std::tie(dev, kind, stream, P, M, W, H, reserve, flags) <
               std::tie(o.dev, o.kind, o.stream, o.P, o.M, o.W, o.H, o.reserve, o.flags);
    }
};
struct GraphCtx {
    void* d_args = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraphNode_t node0 = nullptr;
    hipKernelNodeParams node0_params = {};
    uint64_t last_use = 0;
    bool pinned = false;   // a caller's captured graph refers to d_args (launch_graph): never evicted
};
std::mutex g_ctx_mu;
std::map<CtxKey, GraphCtx> g_graphs;
std::map<std::tuple<int, int, hipStream_t>, void*> g_direct_blocks;   // (device, kind, stream) -> device block
std::unordered_map<int, hipStream_t> g_capture_streams;
uint64_t g_use_clock = 0;
constexpr size_t kMaxGraphs = 48;

void* direct_block(int dev, int kind, hipStream_t s, size_t bytes)
{
    void*& p = g_direct_blocks[{dev, kind, s}];
    if (!p) R3_HIP(hipMalloc(&p, bytes));
    return p;
}

hipStream_t capture_stream(int dev)
{
    hipStream_t& s = g_capture_streams[dev];
    if (!s) R3_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}

void evict_graphs_locked()
{
    while (g_graphs.size() > kMaxGraphs) {
        auto victim = g_graphs.end();
        for (auto it = g_graphs.begin(); it != g_graphs.end(); ++it)
            if (!it->second.pinned && (victim == g_graphs.end() || it->second.last_use < victim->second.last_use)) victim = it;
        if (victim == g_graphs.end()) return;   // every entry is held by a caller's graph
        // the exec may still be queued on its stream: wait for that stream before tearing it down (rare path)
        (void)hipStreamSynchronize(victim->first.stream);
        if (victim->second.exec) (void)hipGraphExecDestroy(victim->second.exec);
        if (victim->second.graph) (void)hipGraphDestroy(victim->second.graph);
        if (victim->second.d_args) (void)hipFree(victim->second.d_args);
        g_graphs.erase(victim);
    }
}

bool graphs_enabled()
{
    static const bool on = !env_is("R3DGS_GRAPH", "0");
    return on;
}

// ---- the launch chains -----------------------------------------------------------------------------------------------
struct NoHooks {
    void begin(int, hipStream_t) {}
    void end(int, const char*, hipStream_t) {}
};

// phases: 1 = geometry (+ header: everything num_rendered depends on), 2 = the rest.  The geometry kernel installs the
// pass block `args` at `d` for the kernels behind it; a caller that issues phase 2 on its own (exact-size path) writes
// the completed block with write_args first.
template <class Hooks>
void issue_forward(const FwdPlan& p, FwdPassArgs* d, const FwdPassArgs& args, hipStream_t s, int phases, Hooks& h,
                   GeomState* g_host)
{
    if (phases & 1) {
        h.begin(kPre, s);
        issue_preprocess_geom(p, d, args, s);
        h.end(kPre, "preprocess", s);
        if (!args.depth.fuse_header) issue_header_reduce(&d->header, s);
    }
    if (phases & 2) {
        h.begin(kDepthSort, s);
        if (p.generic_depth_sort)
            run_generic_depth_sort(p.P, *g_host, s);
        else
            issue_depth_sort_and_color(p, d, s);   // the SH -> RGB stream rides in spare workgroups of these kernels
        h.end(kDepthSort, "depth sort + scan", s);
        if (p.generic_depth_sort) {   // no sort kernel of ours to carry the colour chunks
            h.begin(kColor, s);
            issue_preprocess_color(p, &d->pre, s);
            h.end(kColor, "SH colours", s);
        }
        h.begin(kBinning, s);
        issue_tile_binning(p, d, s);
        h.end(kBinning, "tile binning", s);
        h.begin(kBlendFwd, s);
        issue_blend_forward(p, &d->blend, s);
        h.end(kBlendFwd, "blend forward", s);
    }
}

template <class Block>
void launch_write_args(Block* dst, const Block& v, hipStream_t s);

// The backward blend installs the pass block; without pairs (empty reservation) it does not run and write_args does.
template <class Hooks>
void issue_backward(const BwdPlan& p, BwdPassArgs* d, const BwdPassArgs& args, hipStream_t s, Hooks& h)
{
    h.begin(kBlendBwd, s);
    // the pair flags are all zero here: the forward's tile_ranges kernel clears them and pair_reduce puts every
    // flag it consumed back to zero, so neither pass pays for a fill of its own
    if (p.has_pairs) {
        issue_unit_order(p, d, args, s);
        h.begin(kBlendBwdKernel, s);
        issue_blend_backward(p, d, args, s);
        h.end(kBlendBwdKernel, "blend backward kernel", s);
        if (p.absgrad) issue_absgrad_reduce(p, d, s);   // reads the pair flags pair_reduce clears
        issue_pair_reduce(p, &d->reduce, s);
    } else {
        launch_write_args(d, args, s);
        if (p.absgrad) issue_absgrad_reduce(p, d, s);   // nothing was binned: zeros
    }
    h.end(kBlendBwd, "blend backward", s);
    h.begin(kPreBwd, s);
    issue_preprocess_backward(p, &d->pre, s);
    h.end(kPreBwd, "preprocess backward", s);
}

template <class Block>
void launch_write_args(Block* dst, const Block& v, hipStream_t s)
{
    hipLaunchKernelGGL(write_args_kernel<Block>, dim3(1), dim3(256), 0, s, dst, v);
}

// Replays (capturing it first if this shape is new) the launch chain of a pass as one graph launch on `s`.  Node 0 of
// the chain is the kernel that receives (Block* dst, Block by value) and installs the block; on replay only its
// arguments are refreshed (hipGraphExecKernelNodeSetParams copies them at the call, so a host running many passes
// ahead cannot disturb launches that are still queued -- checked in tools/launch_bench2.hip with the GPU kept busy).
template <class Block, class Plan, class IssueFn>
void launch_graph(const CtxKey& key, const Plan& plan, const Block& args, hipStream_t s, IssueFn&& issue)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    // Is the caller capturing `s` into a graph of its own (torch.cuda.graph)?  (The null stream cannot be captured, and is what a
    // trainer usually runs on: nothing is asked for it.)
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (s != nullptr) R3_HIP(hipStreamIsCapturing(s, &capturing));
    if (capturing == hipStreamCaptureStatusActive) {
        // A launch of our exec would enter the caller's graph as a copy of the chain with the arguments of the pass it was
        // captured from.  The chain goes into the caller's graph as it is instead, with THIS pass's block in its first node.
        // The shape's block must exist already -- nothing may be allocated or captured inside the caller's capture -- and
        // stays for good from here on: the caller's graph refers to it for as long as it is replayed.
        auto it = g_graphs.find(key);
        if (it == g_graphs.end() || !it->second.exec)
            throw Error("this pass is being captured into a graph of the caller's, but its shape has not run on this stream "
                        "yet: run the step once on the stream before capturing it (warm-up)");
        it->second.pinned = true;
        it->second.last_use = ++g_use_clock;
        issue(plan, static_cast<Block*>(it->second.d_args), args, s);
        return;
    }
    GraphCtx& c = g_graphs[key];
    if (!c.exec) {
        try {
            R3_HIP(hipMalloc(&c.d_args, sizeof(Block)));
            hipStream_t cap = capture_stream(key.dev);
            R3_HIP(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
            try {
                issue(plan, static_cast<Block*>(c.d_args), args, cap);
            } catch (...) {
                hipGraph_t dead = nullptr;
                (void)hipStreamEndCapture(cap, &dead);
                if (dead) (void)hipGraphDestroy(dead);
                throw;
            }
            R3_HIP(hipStreamEndCapture(cap, &c.graph));
            size_t n_root = 0;
            R3_HIP(hipGraphGetRootNodes(c.graph, nullptr, &n_root));
            if (n_root != 1) throw Error("captured pass graph is not a linear chain");
            R3_HIP(hipGraphGetRootNodes(c.graph, &c.node0, &n_root));
            R3_HIP(hipGraphKernelNodeGetParams(c.node0, &c.node0_params));
            R3_HIP(hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0));
            c.last_use = ++g_use_clock;   // before the eviction below: the newest entry must not be its victim
        } catch (...) {
            if (c.graph) (void)hipGraphDestroy(c.graph);
            if (c.d_args) (void)hipFree(c.d_args);
            g_graphs.erase(key);
            throw;
        }
        evict_graphs_locked();
    }
    GraphCtx& ctx = g_graphs[key];
    ctx.last_use = ++g_use_clock;
    Block* dst = static_cast<Block*>(ctx.d_args);
    Block copy = args;
    void* params[2] = {&dst, &copy};
    hipKernelNodeParams kp = ctx.node0_params;   // function, grid, block as captured
    kp.kernelParams = params;
    kp.extra = nullptr;
    R3_HIP(hipGraphExecKernelNodeSetParams(ctx.exec, ctx.node0, &kp));   // by-value block: copied at this call
    R3_HIP(hipGraphLaunch(ctx.exec, s));
}

// ---- argument blocks -------------------------------------------------------------------------------------------------
void validate_forward(const FwdCall& c)
{
    if (c.quantised) {
        const QuantInputs& q = c.quant;
        if (!q.xyz || !q.geom_ids || !q.sh_ids || !q.codebooks || !c.viewmatrix || !c.projmatrix || !c.cam_pos || !c.background ||
            !c.out_color)
            throw Error("a required pointer is NULL");
        // what the kernels' loads assume: one 8-byte load of a Gaussian's geometry ids, dwordx4 loads of the codebooks
        if (reinterpret_cast<uintptr_t>(q.geom_ids) % 8 || reinterpret_cast<uintptr_t>(q.codebooks) % 16 ||
            reinterpret_cast<uintptr_t>(q.xyz) % (q.xyz_is_half ? 2 : 4))
            throw Error("quantised model: geom_ids must be 8-byte aligned, codebooks 16-byte, xyz to its element");
    } else {
        if (!c.means3D || !c.opacities || !c.viewmatrix || !c.projmatrix || !c.cam_pos || !c.background || !c.out_color)
            throw Error("a required pointer is NULL");
        if (!c.colors_precomp && !c.shs) throw Error("provide SHs or precomputed colours");
        if (!c.cov3D_precomp && (!c.scales || !c.rotations)) throw Error("provide scale/rotation or a precomputed 3D covariance");
        if (!c.colors_precomp && !c.coeffsNum && (c.M < 1 || c.M > 16)) throw Error("SH coefficient count M must be in [1,16]");
        if (!c.colors_precomp && !c.coeffsNum && !c.D) throw Error("per-Gaussian degrees must be provided with SHs");
    }
    if (c.width <= 0 || c.height <= 0) throw Error("image size must be positive");
    if (c.calculate_mean_transmittance && (!c.out_touched_pixels || !c.out_transmittance))
        throw Error("counter mode needs out_touched_pixels and out_transmittance");
}

FwdPlan make_fwd_plan(const FwdCall& c, uint32_t reserve)
{
    // workgroups of the colour stream per launch that carries it: P / 512 between 512 and 4096 (measured: 1024 vs 512 at
    // 500 k: stage 0.086 vs 0.088 ms; 4096 vs 512 at 2 M: 0.259 vs 0.299 ms); R3DGS_COLOR_GRID overrides
    static const int color_grid_env = env_int("R3DGS_COLOR_GRID", -1, 0, 1 << 20);
    static const bool generic_env = env_is("R3DGS_DEPTH_SORT", "generic");   // forces the rocPRIM path (A/B runs, tests)
    FwdPlan p;
    p.P = c.P;
    p.M = c.M;
    p.W = c.width;
    p.H = c.height;
    const TileGrid grid = grid_of(c.width, c.height);
    p.gx = (int)grid.gx;
    p.gy = (int)grid.gy;
    p.reserve = reserve;
    p.grid_pairs = grid_pairs_for(reserve);
    p.layout = pair_layout(c.P, grid.n());
    p.nb = depth_bucket_count((size_t)c.P);
    p.ragged = (c.coeffsNum != nullptr && !c.colors_precomp) ? 1 : 0;
    p.counters = c.calculate_mean_transmittance ? 1 : 0;
    p.color_grid = color_grid_env >= 0 ? color_grid_env : std::min(4096, std::max(512, c.P / 512));
    // share of the colour chunks carried by the histogram / scatter / bucket-sort launches: 25 / 45 / 30 % up to 1 M Gaussians
    // (round 6, profiles/r06_sweep_colour_split.txt: depth sort + colour 0.0896 against 0.0929 ms with round 5's 20 / 35 / 45 at
    // 500 k, both alternating rounds), 25 / 25 / 50 % above (2 M: stage 0.257 vs 0.266 ms, 6 M: 0.762 vs 0.778)
    static const int split0_env = env_int("R3DGS_COLOR_SPLIT0", -1, 0, 100), split1_env = env_int("R3DGS_COLOR_SPLIT1", -1, 0, 100);
    const bool big = c.P > (1 << 20);
    const int split0 = split0_env >= 0 ? split0_env : 25, split1 = split1_env >= 0 ? split1_env : big ? 25 : 45;
    p.color_split[0] = split0;
    p.color_split[1] = split0 + split1 > 100 ? 100 - split0 : split1;
    p.color_split[2] = 100 - p.color_split[0] - p.color_split[1];
    p.generic_depth_sort = (generic_env || c.P >= (1 << 24)) ? 1 : 0;   // the bucket histogram packs the count in 24 bits
    p.tight = tight_rects();
    p.raw_params = c.raw ? 1 : 0;
    p.quant = c.quantised ? 1 : 0;
    return p;
}

void fill_fwd_args(FwdPassArgs& a, const FwdPlan& p, const FwdCall& c, const GeomState& g, const BinState* b,
                   const ImageState& img, PassInfo* info_dev, uint64_t ticket, bool fuse_header)
{
    memset(&a, 0, sizeof(a));
    int* radii = c.radii ? c.radii : g.radii_internal;
    FwdInputs& in = a.pre.in;
    in.P = c.P;
    in.M = c.M;
    in.degrees = c.D;
    in.means3D = c.means3D;
    in.scales = c.scales;
    in.rotations = c.rotations;
    in.opacities = c.opacities;
    in.shs = c.shs;
    in.cov3D_precomp = c.cov3D_precomp;
    in.colors_precomp = c.colors_precomp;
    in.coeffs_num = p.ragged ? c.coeffsNum : nullptr;
    in.per_band_count = p.ragged ? c.perBand : nullptr;
    in.cumsum_count = p.ragged ? c.cumSum : nullptr;
    a.shs_rest = c.raw ? c.shs_rest : nullptr;
    if (c.quantised) a.quant = c.quant;
    ViewParams& v = a.pre.view;
    v.view = c.viewmatrix;
    v.proj = c.projmatrix;
    v.campos = c.cam_pos;
    v.bg = c.background;
    v.tan_fovx = c.tan_fovx;
    v.tan_fovy = c.tan_fovy;
    v.W = c.width;
    v.H = c.height;
    v.scale_modifier = c.scale_modifier;
    a.pre.rec = g.rec;
    a.pre.rect = g.rect;
    a.pre.depth_key = g.depth_key;
    a.pre.tiles = g.tiles;
    a.pre.partials = g.partials;
    a.pre.radii = radii;
    a.pre.color_blocks = (c.P + kPreBlockSize - 1) / kPreBlockSize;
    a.pre.tight = p.tight;
    // (a forward that its caller knows no backward will follow -- r3dgs_forward_hint(0) -- leaves nothing; the header says so)
    a.pre.sh_ddir = (g_next_forward_trains && !p.ragged && c.shs && !c.colors_precomp) ? g.sh_ddir : nullptr;

    a.header.parts = g.partials;
    a.header.n_parts = (int)pre_partials((size_t)c.P);
    a.header.hdr = g.header;
    a.header.info = info_dev;
    a.header.ticket = (uint32_t)ticket_number(ticket);
    a.header.reserve = p.reserve;
    a.header.stamp_sort = p.generic_depth_sort ? 1 : 0;   // no scan kernel behind the header on the generic-sort route
    a.header.sh_cache = a.pre.sh_ddir ? 1u : 0u;
    // checkpoints for a split backward walk: only a forward that a backward will follow leaves them
    // (the header is written in the exact-size path's first phase, before the binning blob exists: what it says must not
    // depend on `b`)
    const bool leave_ckpt = g_next_forward_trains && bwd_segments() && !p.counters;
    float4* const ckpt = (b && leave_ckpt) ? b->ckpt : nullptr;
    a.header.ckpt = leave_ckpt ? (uint32_t)bwd_segment_log2() : 0u;
    a.header.ckpt_factor_pct = (uint32_t)bwd_segment_factor_pct();
    a.header.n_tiles = (uint32_t)(p.gx * p.gy);

    DepthArgs& d = a.depth;
    d.P = c.P;
    d.nb = p.nb;
    d.rows = (int)depth_hist_rows((size_t)c.P);
    d.per_block = (int)depth_hist_per_block((size_t)c.P);
    d.fuse_header = fuse_header ? 1 : 0;
    d.key = g.depth_key;
    d.tiles = g.tiles;
    d.hdr = g.header;
    d.info = info_dev;
    d.ticket = (uint32_t)ticket_number(ticket);
    d.ds = g.dsort;
    d.hist_rows = g.hist_rows;
    d.hist_base = g.hist_base;
    d.key_sorted = g.key_sorted;
    d.bucket_id = g.bucket_id;
    d.ovf_key = g.ovf_key;
    d.ovf_id = g.ovf_id;
    d.rect = g.rect;
    d.rec16 = g.rec16;
    d.rec16_b = g.rec16_b;
    d.rect_sorted = g.rect_sorted;
    d.order = g.order;
    d.offsets = g.offsets;
    // only on the asynchronous path does the binning blob exist while the depth sort runs (and only the bucketed sort's
    // scan writes the notes)
    uint32_t* const block_first = (b && fuse_header && !p.generic_depth_sort) ? b->block_first : nullptr;
    d.block_first = block_first;
    d.block_cap = p.reserve / (uint32_t)kRadixBlock + 2u;

    const PairLayout& l = p.layout;
    const size_t Tn = (size_t)p.gx * p.gy;
    if (b) {
        const uint32_t stride = radix_row_stride(p.reserve);
        EmitArgs& e = a.emit;
        e.P = c.P;
        e.gx = p.gx;
        e.hdr = g.header;
        e.order = g.order;
        e.offsets = g.offsets;
        e.block_first = block_first;
        e.rect = g.rect;
        e.rect_sorted = p.generic_depth_sort ? nullptr : g.rect_sorted;
        e.rec = g.rec;
        e.rank_bits = l.rank_bits;
        e.digit_bits = l.digit_bits;
        e.words_out = b->words_a;
        e.cap = p.reserve;
        e.pair_rank = l.wide == 1 ? b->pair_rank : nullptr;
        e.ranges = img.ranges;
        e.n_tiles = (uint32_t)Tn;
        e.radix_rows = b->radix_rows;
        e.row_stride = stride;
        // buffer chain of the passes: narrow a -> b -> c (-> b), wide a -> b -> a (-> b); words_a of the narrow layout
        // survives for the backward (pair_rank aliases it)
        const char* src = b->words_a;
        for (int k = 0; k < l.passes; k++) {
            char* dst = l.wide ? ((k & 1) ? b->words_a : b->words_b) : ((k & 1) ? b->words_c : b->words_b);
            RadixArgs& r = a.radix[k];
            r.hdr = g.header;
            r.in = src;
            r.out = dst;
            r.ids_out = (l.wide == 2 && k == l.passes - 1) ? b->point_list : nullptr;
            r.cap = p.reserve;
            r.shift = l.rank_bits + k * l.digit_bits;
            r.digit_bits = l.digit_bits;
            r.rank_bits = l.rank_bits;
            r.tile_shift = k * l.digit_bits;
            r.rows = b->radix_rows;
            r.base = b->radix_base;
            r.total = b->radix_total + k * kMaxRadixBins;
            r.row_stride = stride;
            src = dst;
        }
        if (src != sorted_words(*b, l)) throw Error("internal: sorted-word buffer mismatch");
        RangesArgs& t = a.ranges;
        t.hdr = g.header;
        t.sorted = src;
        t.cap = p.reserve;
        t.rank_bits = l.rank_bits;
        t.order = nullptr;   // the words carry Gaussian ids
        t.point_list = b->point_list;
        t.ranges = img.ranges;
        t.pair_flag = b->pair_flag;
    }
    BlendFwdArgs& f = a.blend;
    f.ranges = img.ranges;
    f.point_list = b ? b->point_list : nullptr;
    f.rec = g.rec;
    f.W = c.width;
    f.H = c.height;
    f.gx = p.gx;
    f.nblocks = (uint32_t)(p.gx * p.gy * 4);
    f.bg = c.background;
    f.out_color = c.out_color;
    f.final_T = img.final_T;
    f.n_contrib = img.n_contrib;
    f.touched = p.counters ? c.out_touched_pixels : nullptr;
    f.transmittance = p.counters ? c.out_transmittance : nullptr;
    f.quad_masks = b && keep_quad_masks() ? b->quad_masks : nullptr;
    f.quad_depth = img.quad_depth;
    f.ckpt = ckpt;
    f.hdr = g.header;
}

uint32_t fwd_flags(const FwdPlan& p, const FwdCall& c)
{
    return (uint32_t)p.ragged | ((uint32_t)p.counters << 1) | ((uint32_t)(c.colors_precomp != nullptr) << 2) |
           ((uint32_t)p.tight << 3) | ((uint32_t)p.raw_params << 4) | ((uint32_t)p.layout.wide << 5) |   // wide: 0 / 1 / 2
           ((uint32_t)p.quant << 7);
}

uint64_t new_ticket(int dev, const FwdCall& c, uint32_t reserve, bool sort_stamp, PassInfo** info_dev)
{
    const uint64_t number = g_next_ticket.fetch_add(1);
    const uint64_t ticket = make_ticket(dev, number);
    InfoRing& ring = info_ring(dev);
    *info_dev = ring.dev + number % kInfoRing;
    g_adv.note_pass({ticket, dev, c.P, c.width, c.height, reserve, reinterpret_cast<uintptr_t>(c.viewmatrix), sort_stamp});
    return ticket;
}

template <class Block>
Block* direct_args(int dev, int kind, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    return static_cast<Block*>(direct_block(dev, kind, s, sizeof(Block)));
}

void validate_backward(const BwdCall& c)
{
    if (c.absgrad) check_absgrad_args(c.R, c.blobs.binning != nullptr, c.dL_dmean2D_abs, c.abs_workspace, c.abs_workspace_floats);
    if (!c.blobs.geom || !c.blobs.image) throw Error("state buffers must not be NULL");
    if (!c.means3D || !c.viewmatrix || !c.projmatrix || !c.campos || !c.background || !c.dL_dpix)
        throw Error("a required pointer is NULL");
    if (!c.dL_dmean2D || !c.dL_dopacity || !c.dL_dcolor || !c.dL_dmean3D || !c.dL_dcov3D || !c.dL_dscale || !c.dL_drot)
        throw Error("a gradient output pointer is NULL");
    if (c.shs && (!c.dL_dsh || !c.D || c.M < 1 || c.M > 16)) throw Error("SH gradients need dL_dsh, degrees and 1 <= M <= 16");
}

BwdPlan make_bwd_plan(const BwdCall& c)
{
    const TileGrid grid = grid_of(c.width, c.height);
    BwdPlan p;
    p.P = c.P;
    p.M = c.M;
    p.W = c.width;
    p.H = c.height;
    p.gx = (int)grid.gx;
    p.gy = (int)grid.gy;
    p.layout = pair_layout(c.P, grid.n());
    // R: the pair capacity the forward carved the binning blob with (num_rendered of an exact-size forward, the
    // reservation of a reserved one); the pair count itself is read from the device header
    p.reserve = c.R > 0 ? (uint32_t)c.R : 1u;
    p.grid_pairs = grid_pairs_for(p.reserve);
    p.has_pairs = c.blobs.binning != nullptr ? 1 : 0;
    p.units_cap = bwd_units_cap(p.reserve, grid);
    p.f64_chain = f64_chain();
    p.raw_params = c.raw ? 1 : 0;
    p.absgrad = c.absgrad ? 1 : 0;
    return p;
}

void fill_bwd_args(BwdPassArgs& a, const BwdPlan& plan, const BwdCall& c, const PassStates& st)
{
    const GeomState& geom = st.geom;
    const BinState& bin = st.bin;
    const ImageState& img = st.img;
    memset(&a, 0, sizeof(a));
    BlendBwdArgs& bb = a.blend;
    bb.ranges = img.ranges;
    bb.point_list = bin.point_list;
    bb.rec = geom.rec;
    bb.final_T = img.final_T;
    bb.n_contrib = img.n_contrib;
    bb.dL_dpix = c.dL_dpix;
    bb.W = c.width;
    bb.H = c.height;
    bb.gx = plan.gx;
    bb.nblocks = (uint32_t)(plan.gx * plan.gy);   // one wave per tile: the per-pair gradient slab has ONE owner per (tile, Gaussian)
    bb.bg = c.background;
    bb.pair_grad = bin.pair_grad;
    bb.pair_flag = bin.pair_flag;
    bb.quad_masks = plan.has_pairs && keep_quad_masks() ? bin.quad_masks : nullptr;
    // the unit order lives in the binning blob: a pass without one (no pair was reserved) has nothing to order; a unit
    // word holds kUnitTileBits of tile index (an image of more than 2^20 tiles -- 268 Mpix -- is walked row-major)
    bb.unit_order = (heaviest_tiles_first() && plan.has_pairs && (size_t)plan.gx * plan.gy <= ((size_t)1 << kUnitTileBits))
                        ? bin.unit_order : nullptr;
    bb.units_cap = plan.units_cap;
    bb.quad_depth = img.quad_depth;
    bb.ckpt = plan.has_pairs ? bin.ckpt : nullptr;
    bb.hdr = geom.header;
    bb.segments = bwd_segments();
    PairReduceArgs& pr = a.reduce;
    pr.hdr = geom.header;
    pr.pair_grad = bin.pair_grad;
    pr.pair_flag = bin.pair_flag;
    pr.pair_rank = bin.pair_rank;
    pr.rank_mask = plan.layout.wide ? 0xFFFFFFFFu : (1u << plan.layout.rank_bits) - 1u;
    pr.order = nullptr;   // the run key is the Gaussian id itself
    pr.rec = geom.rec;
    pr.tiles = geom.tiles;
    pr.acc = geom.acc;
    pr.wave_part = bin.wave_part;
    {   // this pass's stamp: a 64-bit counter that starts at a random value per process -- no row left by an earlier
        // pass of this or of another process (recycled device memory) can carry it
        static std::atomic<unsigned long long> stamp{[] {
            std::random_device rd;
            return ((unsigned long long)rd() << 32) ^ (unsigned long long)rd() ^ 0x9E3779B97F4A7C15ull;
        }()};
        const unsigned long long st64 = stamp.fetch_add(1);
        pr.stamp0 = (uint32_t)st64;
        pr.stamp1 = (uint32_t)(st64 >> 32);
    }
    PreBwdArgs& pb = a.pre;
    FwdInputs& in = pb.in;
    in.P = c.P;
    in.M = c.M;
    in.degrees = c.D;
    in.means3D = c.means3D;
    in.scales = c.scales;
    in.rotations = c.rotations;
    in.opacities = nullptr;
    in.shs = c.colors_precomp ? nullptr : c.shs;
    in.cov3D_precomp = c.cov3D_precomp;
    in.colors_precomp = c.colors_precomp;
    ViewParams& view = pb.view;
    view.view = c.viewmatrix;
    view.proj = c.projmatrix;
    view.campos = c.campos;
    view.bg = c.background;
    view.tan_fovx = c.tan_fovx;
    view.tan_fovy = c.tan_fovy;
    view.W = c.width;
    view.H = c.height;
    view.scale_modifier = c.scale_modifier;
    pb.radii = c.radii ? c.radii : geom.radii_internal;
    pb.rec = geom.rec;
    pb.tiles = geom.tiles;
    pb.acc = geom.acc;
    pb.wave_part = plan.has_pairs ? bin.wave_part : nullptr;
    pb.stamp0 = pr.stamp0;
    pb.stamp1 = pr.stamp1;
    pb.header = geom.header;
    pb.lambda_sh = c.lambda_sh_sparsity;
    pb.sh_ddir = (c.lambda_sh_sparsity == 0.f && sh_derivative_cache()) ? geom.sh_ddir : nullptr;
    pb.out.dL_dmean2D = c.dL_dmean2D;
    pb.out.dL_dopacity = c.dL_dopacity;
    pb.out.dL_dcolor = c.dL_dcolor;
    pb.out.dL_dmean3D = c.dL_dmean3D;
    pb.out.dL_dcov3D = c.dL_dcov3D;
    pb.out.dL_dsh = c.dL_dsh;
    pb.shs_rest = c.raw ? c.shs_rest : nullptr;
    pb.dL_dsh_rest = c.raw ? c.dL_dsh_rest : nullptr;
    pb.out.dL_dscale = c.dL_dscale;
    pb.out.dL_drot = c.dL_drot;
    pb.out.dL_dconic = c.dL_dconic;
    static const int stagger = env_int("R3DGS_PREBWD_STAGGER", 127, 0, 4096);   // 0 / 64 / 127 / 254 / 508:
                                                                                 // 84.0 / 79.5 / 79.8 / 79.7 / 88.6 us
    pb.stagger = stagger;
    if (plan.absgrad) {
        a.abs.out = c.dL_dmean2D_abs;
        a.abs.workspace = c.abs_workspace;
    }
}

uint32_t bwd_flags(const BwdPlan& p, const BwdPassArgs& a)
{
    return ((uint32_t)p.has_pairs << 3) | ((uint32_t)p.layout.wide << 4) |
           ((uint32_t)(a.blend.unit_order != nullptr) << 6) |   // one more kernel in the chain
           ((uint32_t)p.f64_chain << 7) | ((uint32_t)p.raw_params << 8) |
           ((uint32_t)p.absgrad << 9);   // the abs pass is a chain of its own: other blend instantiations, three more kernels
}

}  // namespace

namespace r3 {

int last_forward_pairs() { return g_last_forward_pairs; }
void set_forward_trains(int trains) { g_next_forward_trains = trains; }

const volatile PassInfo* pass_info(long long ticket, int wait)
{
    if (ticket <= 0) throw Error("not a pass ticket");
    const uint64_t t = (uint64_t)ticket, n = ticket_number(t);
    if (g_next_ticket.load() - n >= kInfoRing) throw Error("pass ticket expired (ring reused)");
    // the ring of the device the pass ran on (carried by the ticket), whatever device is current here
    const volatile PassInfo* info = info_ring(ticket_device(t)).host + n % kInfoRing;
    if (wait)
        info = wait_info(t);
    else if (info->seq != (uint32_t)n)
        return nullptr;
    std::atomic_thread_fence(std::memory_order_acquire);
    return info;
}

uint32_t reserve_hint(int P, int W, int H, const float* viewmatrix)
{
    static const bool off = env_is("R3DGS_RESERVE", "off");
    static const double slack = 0.01 * env_int("R3DGS_RESERVE_SLACK_PCT", 150, 100, 1600);
    const int dev = current_device();
    if (off) return 0;
    return g_adv.hint(dev, P, W, H, reinterpret_cast<uintptr_t>(viewmatrix), slack, g_next_ticket.load(), pass_published);
}
void reserve_forget_view(const float* viewmatrix) { g_adv.forget_view(reinterpret_cast<uintptr_t>(viewmatrix)); }
void reserve_forget_all() { g_adv.forget_all(); }
long long reserve_overflow_events(int* last_num_rendered, int* last_reserve)
{
    uint32_t rendered = 0, reserve = 0;
    const uint64_t events = g_adv.overflow_events(g_next_ticket.load(), pass_published, &rendered, &reserve);
    if (last_num_rendered) *last_num_rendered = (int)rendered;
    if (last_reserve) *last_reserve = (int)reserve;
    return (long long)events;
}

void profile_enable(int on)
{
    // on == 0: off; on == 1: every stage; otherwise bit (s + 1) of `on` selects stage s alone.  A pass with a timed
    // stage is issued with direct launches (events sit between its kernels); the other pass keeps its graph.
    g_prof.mask.store(on == 0 ? 0u : (on == 1 ? ((1u << kNumStages) - 1u) : (((unsigned)on >> 1) & ((1u << kNumStages) - 1u))));
}

void profile_read(double* total_ms, int* launches)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (int st = 0; st < kNumStages; st++) {
        double sum = 0.0;
        for (auto& ev : g_prof.used[st]) {
            R3_HIP(hipEventSynchronize(ev.second));
            float ms = 0.f;
            R3_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
            sum += ms;
            g_prof.pool.push_back(ev.first);
            g_prof.pool.push_back(ev.second);
        }
        if (total_ms) total_ms[st] = sum;
        if (launches) launches[st] = (int)g_prof.used[st].size();
        g_prof.used[st].clear();
    }
}

int forward_exact(const Allocators& alloc, const FwdCall& c)
{
    g_last_forward_pairs = 0;
    if (c.P <= 0) return 0;
    if (!alloc.geometry || !alloc.binning || !alloc.image) throw Error("allocator callbacks must not be NULL");
    validate_forward(c);
    hipStream_t s = c.stream;
    const int dev = current_device();
    FwdPlan plan = make_fwd_plan(c, 0xFFFFFFFFu);
    if (!plan.generic_depth_sort && g_adv.take_prefer_generic(dev, c.width, c.height)) plan.generic_depth_sort = 1;
    prepare_depth_bucket_sort(plan.nb);
    const size_t depth_temp = cached_depth_temp((size_t)c.P);
    const bool lean = !(g_next_forward_trains && !plan.ragged && c.shs && !c.colors_precomp);   // no sh_ddir will be written
    char* gptr = alloc.geometry(geometry_blob_bytes((size_t)c.P, depth_temp, lean), alloc.geometry_user);
    if (!gptr) throw Error("geometry allocator returned NULL");
    GeomState geom = GeomState::carve(gptr, (size_t)c.P, depth_temp);
    const TileGrid grid = grid_of(c.width, c.height);
    const size_t N = (size_t)c.width * c.height;
    char* iptr = alloc.image(required_bytes<ImageState>(N, grid.n()), alloc.image_user);
    if (!iptr) throw Error("image allocator returned NULL");
    ImageState img = ImageState::carve(iptr, N, grid.n());

    PassInfo* info_dev = nullptr;
    const uint64_t ticket = new_ticket(dev, c, 0xFFFFFFFFu, false, &info_dev);
    FwdPassArgs* d_args;
    StageRun hooks{c.debug != 0};
    FwdPassArgs args;
    try {
        d_args = direct_args<FwdPassArgs>(dev, 0, s);
        fill_fwd_args(args, plan, c, geom, nullptr, img, info_dev, ticket, false);
        issue_forward(plan, d_args, args, s, 1, hooks, &geom);
    } catch (...) {
        g_adv.forget_ticket(ticket);
        throw;
    }
    // the one structural wait of this entry point (the reference's cudaMemcpy at rasterizer_impl.cu:446)
    const volatile PassInfo* info = wait_info(ticket);
    const uint32_t R = info->pairs, R_ref = info->num_rendered;
    if (R > 0x7fffffffu || R_ref > 0x7fffffffu) throw Error("num_rendered exceeds 2^31-1");
    g_last_forward_pairs = (int)R;
    // The blob is carved for the count this entry point RETURNS (the reference's num_rendered, >= the pairs binned with the
    // opacity-aware rects): a caller that follows the reference's contract hands that number to r3dgs_backward /
    // r3dgs_export_binning as R, and both carve the blob with it.  Grids are sized by the pairs.
    plan.reserve = R_ref ? R_ref : 1u;
    plan.grid_pairs = R ? R : 1u;     // exact size: one block per chunk
    char* bptr = alloc.binning(required_bytes<BinState>((size_t)plan.reserve, plan.layout.wide, grid), alloc.binning_user);
    if (!bptr) throw Error("binning allocator returned NULL");
    BinState bin = BinState::carve(bptr, (size_t)plan.reserve, plan.layout.wide, grid);
    fill_fwd_args(args, plan, c, geom, &bin, img, info_dev, ticket, false);
    launch_write_args(d_args, args, s);   // the completed block (binning pointers, pair capacity)
    issue_forward(plan, d_args, args, s, 2, hooks, &geom);
    return (int)R_ref;   // what the reference returns: the tile count of ITS rects (== R with the tight rects off)
                         // == the capacity the binning blob was carved with
}

long long forward_reserved(const PassBlobs& blobs, int reserve, const FwdCall& c)
{
    if (c.P <= 0) return 0;
    if (reserve < 1) throw Error("the pair reservation must be >= 1");
    if (!blobs.geom || !blobs.binning || !blobs.image) throw Error("state buffers must not be NULL");
    validate_forward(c);
    hipStream_t s = c.stream;
    const int dev = current_device();
    FwdPlan plan = make_fwd_plan(c, (uint32_t)reserve);
    if (!plan.generic_depth_sort && g_adv.take_prefer_generic(dev, c.width, c.height)) plan.generic_depth_sort = 1;
    prepare_depth_bucket_sort(plan.nb);
    PassStates st = carve_pass(c.P, plan.reserve, c.width, c.height, blobs, cached_depth_temp((size_t)c.P));
    PassInfo* info_dev = nullptr;
    const uint64_t ticket = new_ticket(dev, c, plan.reserve, !plan.generic_depth_sort, &info_dev);
    try {
        FwdPassArgs args;
        // the generic (rocPRIM) depth sort has no histogram kernel to carry the header reduction
        fill_fwd_args(args, plan, c, st.geom, &st.bin, st.img, info_dev, ticket, !plan.generic_depth_sort);
        const bool direct = !graphs_enabled() || c.debug || plan.generic_depth_sort || (g_prof.mask.load() & kFwdStages);
        if (direct) {
            StageRun hooks{c.debug != 0};
            issue_forward(plan, direct_args<FwdPassArgs>(dev, 0, s), args, s, 3, hooks, &st.geom);
        } else {
            const CtxKey key{dev, 0, s, c.P, c.M, c.width, c.height, plan.reserve, fwd_flags(plan, c)};
            launch_graph(key, plan, args, s, [](const FwdPlan& p, FwdPassArgs* d, const FwdPassArgs& v, hipStream_t cs) {
                NoHooks nh;
                issue_forward(p, d, v, cs, 3, nh, nullptr);
            });
        }
    } catch (...) {
        g_adv.forget_ticket(ticket);
        throw;
    }
    return (long long)ticket;
}

int backward_pass(const BwdCall& c)
{
    if (c.P <= 0) return 0;
    validate_backward(c);
    hipStream_t s = c.stream;
    const BwdPlan plan = make_bwd_plan(c);
    const int dev = current_device();
    const PassStates st = carve_pass(c.P, plan.reserve, c.width, c.height, c.blobs, cached_depth_temp((size_t)c.P));
    BwdPassArgs a;
    fill_bwd_args(a, plan, c, st);
    const bool direct = !graphs_enabled() || c.debug || (g_prof.mask.load() & kBwdStages);
    if (direct) {
        StageRun hooks{c.debug != 0};
        issue_backward(plan, direct_args<BwdPassArgs>(dev, 1, s), a, s, hooks);
    } else {
        const CtxKey key{dev, 1, s, c.P, c.M, c.width, c.height, plan.reserve, bwd_flags(plan, a)};
        launch_graph(key, plan, a, s, [](const BwdPlan& p, BwdPassArgs* d, const BwdPassArgs& v, hipStream_t cs) {
            NoHooks nh;
            issue_backward(p, d, v, cs, nh);
        });
    }
    return 0;
}

}  // namespace r3


