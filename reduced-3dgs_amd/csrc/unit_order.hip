// unit_order.hip -- the launch order of the backward blend's units: heaviest first (the rule: unit_order.h).
//
// All units are resident at once for the first half of the backward blend and each wave's duration is set by how many share
// its SIMD, so in row-major order the chip drains for the whole second half (profiles/r03_bwd_timeline_row_major.txt: 20
// resident waves per CU for five tenths of a CU's span, then 17, 12, 9, 6, 3); started by decreasing weight, the long walks are
// under way when the short ones fill the gaps (0.367 -> 0.313 ms on the metric shape).  A unit is a tile, or one segment of a
// tile whose list is long and deep (common.h): on a scene with the load of a real capture the heaviest tile walks three times
// the mean and the kernel was as long as that walk.  Weight of a unit = sum over the four quadrants of the entries it will
// visit there (ImageState::quad_depth clamped to the segment).  Tiles nothing contributed to are left out.  Counting sort over
// 1024 weight classes (64 classes: +2 us for the stage, 16: +10, 4: +22), one workgroup per unit list (below); the order inside
// a class is whatever the LDS atomics make it -- every unit's arithmetic is its own, so the gradients do not depend on the
// order (tests/test_gpu_parity.py compares the two orders bit for bit).  The hardware deals consecutive workgroups over the
// eight XCDs: as ONE sorted list every XCD got every eighth unit -- equal work per XCD, and every XCD's L2 saw every Gaussian's
// record (FETCH_SIZE 62 -> 150 MB); keeping each XCD on a BAND of the image and ordering inside the band only (74 MB)
// measured 0.315 ms against 0.305 ms for the stage.  The eight lists of 4 x 4 tile blocks (common.h TileGrid) are the
// middle: each XCD walks blocks from all over the image, heaviest first, and neighbouring tiles stay on one XCD.
#include "common.h"
#include "unit_order.h"

namespace r3 {

// In place: the inclusive prefix sum of `incl` over the wave (lane 63 holds the total).  The one statement of the scan, and a
// macro on purpose: as a function or a lambda shared by the full-segment prefix and the class scan the same loop comes out of
// the compiler in another instruction order (a third of the kernel's lines move, one SGPR fewer); expanded in place the
// kernel is the one that was measured, instruction for instruction (profiles/unit_order_split_ab.txt).
#define R3_WAVE_SCAN(incl, lane_id)                                      \
    for (int off = 1; off < 64; off <<= 1) {                            \
        const uint32_t up = (uint32_t)__shfl_up((int)(incl), off);      \
        if ((lane_id) >= (uint32_t)off) (incl) += up;                   \
    }

static_assert(kBwdSegMax < 256, "the kernel keeps a tile's segment count in eight bits");

// KEEP: tiles a thread holds in registers between the passes.  Since the order became kOrderLists lists a thread of the metric
// shape holds ONE tile (864 slots per list), and every further slot still issued its (clamped) loads and its unrolled counting
// code: 12.7 us with eight slots, 7.5 with two (profiles/r05_exp_unit_order.txt); the launch takes the smallest that covers
// the image's longest list (1: <= 1024 slots per list, i.e. up to ~8 k tiles; 2; 8: up to 64 k tiles, beyond that the
// passes re-read).
template <int KEEP>
__global__ __launch_bounds__(kOrderThreads) void unit_order_kernel(BwdPassArgs* dst, BwdPassArgs v)
{
    __shared__ uint32_t s_count[kOrderClasses];
    __shared__ uint32_t s_scan[kOrderThreads / 64];
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x, lane_id = tid & 63u;
    if (blockIdx.x == 0) install_block_from_kernarg(dst, (int)tid, kOrderThreads);   // first kernel of the backward: the pass block
    // One workgroup per LIST: workgroup g orders the tiles of list g (common.h TileGrid: the 4 x 4 tile blocks g, g + lists, ...
    // of the image) with its own class counters, no word exchanged with the others; the blend kernel's workgroup b takes entry
    // b / lists of list b % lists, so the lists are consumed side by side and the launch order is the interleaving of eight
    // orders of statistically alike tile sets.
    // (As ONE workgroup over all tiles the kernel was bound by the vector issue of the one compute unit it ran on: 18 us.)
    const uint32_t list = blockIdx.x, all_tiles = v.blend.nblocks;
    const TileGrid grid{(uint32_t)v.blend.gx, all_tiles / (uint32_t)v.blend.gx};
    const uint4* __restrict__ qd = reinterpret_cast<const uint4*>(v.blend.quad_depth);
    const uint2* __restrict__ ranges = v.blend.ranges;
    uint32_t* __restrict__ order = v.blend.unit_order + unit_list_base(v.blend.units_cap, list);
    uint32_t* __restrict__ trailer = unit_trailer_at(v.blend.unit_order, v.blend.units_cap, list);
    const uint32_t n_tiles = grid.list_slots(list);   // slots of this list; a slot of a block at the image's edge may hold no tile
    auto tile_of = [&](uint32_t j) { return grid.list_tile(list, j); };   // slot -> tile (~0: none)
    const uint32_t seg_log2 = (v.blend.segments != 0 && v.blend.ckpt != nullptr && all_tiles <= (1u << kUnitTileBits))
                                  ? v.blend.hdr->ckpt : 0u;   // 0: the forward left no checkpoints / segments are off
    const uint32_t thr = seg_log2 ? v.blend.hdr->ckpt_thr : 0xFFFFFFFFu;
    // Units a list may hold.  The bound is taken from the pass's pair count, not from the capacity its binning blob happens
    // to have: the exact-size path and the reserved path of one view then walk the same segments and give the same bits.
    const uint32_t fit = bwd_list_fit(v.blend.hdr->num_pairs, grid);   // <= the list's slots: the reservation holds the pairs
    s_count[tid] = 0u;
    if (tid == 0) s_max = 0u;
    __syncthreads();
    // up to KEEP tiles per thread stay in registers between the passes (one memory round trip instead of four: the
    // kernel is a chain of latencies, 9.5 us when every pass went back to memory); a larger grid re-reads
    const bool keep = n_tiles <= (uint32_t)(KEEP * kOrderThreads);
    uint4 w[KEEP];
    uint32_t len[KEEP], tl[KEEP];   // weights, list length and tile of the kept slots
    auto load = [&](uint32_t t, uint4& d, uint32_t& l) {
        d = make_uint4(0u, 0u, 0u, 0u);
        l = 0u;
        const uint32_t tile = t < n_tiles ? tile_of(t) : 0xFFFFFFFFu;
        if (tile != 0xFFFFFFFFu) {
            d = qd[tile];
            const uint2 r = ranges[tile];
            l = r.y - r.x;
        }
    };
    if (keep) {
        // every load in flight before the first use (written as `load` per tile the compiler reused one register pair for the
        // ranges and waited for each of the loads in turn: 12 us of the kernel's 22)
        uint2 rr[KEEP];
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            const uint32_t j = tid + (uint32_t)(k * kOrderThreads);
            tl[k] = j < n_tiles ? tile_of(j) : 0xFFFFFFFFu;
            w[k] = qd[min(tl[k], all_tiles - 1u)];
            rr[k] = ranges[min(tl[k], all_tiles - 1u)];
        }
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            const bool in = tl[k] != 0xFFFFFFFFu;
            if (!in) w[k] = make_uint4(0u, 0u, 0u, 0u);
            len[k] = in ? rr[k].y - rr[k].x : 0u;
        }
    }
    auto wave_prefix = [&](uint32_t x, uint32_t* total) {   // exclusive prefix and total of x over the wave
        uint32_t incl = x;
        R3_WAVE_SCAN(incl, lane_id)
        *total = (uint32_t)__shfl((int)incl, 63);
        return incl - x;
    };
    // (the kernel runs on ONE compute unit per list and is bound by its vector-instruction issue -- integer min / max at half
    // rate -- so nothing is worked out twice: segment counts and the classes of a tile's first three partial segments wait in
    // registers for the placement pass)
    uint32_t nf[KEEP], pc[KEEP];   // segments | full segments << 8, and the cached classes, of the kept tiles
    // The segment length is settled by TRYING: the counting pass runs with the shortest segments (2^seg_log2 entries) and its
    // class scan says how many units that makes; only a pass whose lists are so long that they exceed what the list may
    // launch (tens of millions of pairs: fit = tiles + min(pairs / S, 8 tiles) / lists) counts again with 2 S, 4 S, 8 S and
    // finally whole tiles.  (Round 5 counted the units of all four candidate lengths in a pass of their own before the
    // counting pass, on every backward: 1.3 of the kernel's 12.7 us)
    uint32_t walk = seg_log2, total_units = 0u, full_class = 0u;
    float scale = 0.f;
    for (;;) {
        // The heaviest unit.  A pass that splits knows a bound without looking (unit_order.h).  Without segments: one more pass
        // over the tiles.
        uint32_t heaviest;
        if (walk) {
            heaviest = unit_heaviest_bound(thr, walk);
        } else {
            uint32_t kmax = 0u;
            if (keep) {
#pragma unroll
                for (int k = 0; k < KEEP; k++) kmax = max(kmax, w[k].x + w[k].y + w[k].z + w[k].w);
            } else {
                for (uint32_t t = tid; t < n_tiles; t += kOrderThreads) {
                    uint4 d;
                    uint32_t l;
                    load(t, d, l);
                    kmax = max(kmax, d.x + d.y + d.z + d.w);
                }
            }
            for (int off = 32; off > 0; off >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off));
            if (lane_id == 0u) atomicMax(&s_max, kmax);
            __syncthreads();
            heaviest = s_max;
        }
        scale = unit_class_scale(heaviest);
        // Leading segments of a split tile that all four quadrants walk in full: they all weigh 4 x the segment length -- one
        // class, thousands of units in a deep scene, and one LDS counter they would all queue on (the kernel took 52 us at
        // 2 M Gaussians that way).  A tile's FULL segments are therefore counted and placed as a group, and the groups of the
        // tiles a wave holds at the same step add up among themselves (a shuffle scan): one atomic per wave and step.
        full_class = unit_class(4u << walk, scale);
        // (a) the partial units of a tile: one LDS atomic each; (b) its full segments: the lanes of a wave add theirs up (one
        // shuffle scan per pass over the sum of a thread's tiles) and send one atomic.
        auto count_partials = [&](const uint4& d, uint32_t n, uint32_t f, uint32_t* classes) {
            uint32_t packed = 0u;
            for (uint32_t k = f; k < n; k++) {
                const uint32_t c = unit_class(unit_weight(d, k, n, walk), scale);
                atomicAdd(&s_count[c], 1u);
                if (k - f < kCached) packed |= c << (kClassBits * (k - f));
            }
            *classes = packed;
        };
        if (keep) {
            uint32_t fsum = 0u, total;
#pragma unroll
            for (int k = 0; k < KEEP; k++) {
                const uint32_t n = unit_count(w[k], len[k], thr, walk), f = unit_full_segments(w[k], n, walk);
                nf[k] = n | (f << 8);
                fsum += f;
                count_partials(w[k], n, f, &pc[k]);
            }
            wave_prefix(fsum, &total);
            if (lane_id == 0u && total) atomicAdd(&s_count[full_class], total);
        } else {
            for (uint32_t t0 = 0; t0 < n_tiles; t0 += kOrderThreads) {   // uniform trip count: the wave scan needs every lane
                uint4 d;
                uint32_t l, unused, total;
                load(t0 + tid, d, l);
                const uint32_t n = unit_count(d, l, thr, walk), f = unit_full_segments(d, n, walk);
                count_partials(d, n, f, &unused);
                wave_prefix(f, &total);
                if (lane_id == 0u && total) atomicAdd(&s_count[full_class], total);
            }
        }
        __syncthreads();
        // exclusive scan of the class counts (one class per thread)
        const uint32_t mine = s_count[tid];
        uint32_t incl = mine;
        R3_WAVE_SCAN(incl, lane_id)
        if (lane_id == 63u) s_scan[tid >> 6] = incl;
        __syncthreads();
        uint32_t before = 0u;
        total_units = 0u;
        for (uint32_t k = 0; k < (uint32_t)(kOrderThreads / 64); k++) {
            const uint32_t c = s_scan[k];
            if (k < (tid >> 6)) before += c;
            total_units += c;
        }
        __syncthreads();
        const bool fits = unit_walk_fits(walk, total_units, fit);   // the same for every thread
        s_count[tid] = fits ? before + incl - mine : 0u;       // first slot of the class, then its cursor / cleared for the retry
        if (tid == 0) s_max = 0u;
        __syncthreads();
        if (fits) break;
        walk = unit_next_walk(walk, seg_log2);   // longer segments; none fits: whole tiles
    }
    if (tid == 0) {
        trailer[0] = total_units;   // the units of this list (<= its slots by the choice of `walk`; whole tiles: <= list_tiles_max)
        trailer[1] = walk;          // log2 of the segment length they walk (0: whole tiles)
    }
    auto place = [&](uint32_t tile, const uint4& d, uint32_t n, uint32_t f, uint32_t base, uint32_t classes, bool cached) {
        const uint32_t word = unit_pack(tile, 0u, n);   // the tile's word, its segment field filled in per unit
        for (uint32_t k = 0; k < f; k++) order[base + k] = word | unit_pack(0u, k, 0u);
        for (uint32_t k = f; k < n; k++) {
            const uint32_t c = (cached && k - f < kCached) ? (classes >> (kClassBits * (k - f))) & ((1u << kClassBits) - 1u)
                                                           : unit_class(unit_weight(d, k, n, walk), scale);
            order[atomicAdd(&s_count[c], 1u)] = word | unit_pack(0u, k, 0u);
        }
    };
    auto full_base = [&](uint32_t f) {   // where this lane's full segments go: one atomic per wave
        uint32_t total;
        const uint32_t ahead = wave_prefix(f, &total);
        uint32_t base = 0u;
        if (lane_id == 0u && total) base = atomicAdd(&s_count[full_class], total);
        return (uint32_t)__shfl((int)base, 0) + ahead;
    };
    if (keep) {
        uint32_t fsum = 0u;
#pragma unroll
        for (int k = 0; k < KEEP; k++) fsum += nf[k] >> 8;
        uint32_t base = full_base(fsum);
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            place(tl[k], w[k], nf[k] & 255u, nf[k] >> 8, base, pc[k], true);
            base += nf[k] >> 8;
        }
    } else {
        for (uint32_t t0 = 0; t0 < n_tiles; t0 += kOrderThreads) {
            uint4 d;
            uint32_t l;
            load(t0 + tid, d, l);
            const uint32_t n = unit_count(d, l, thr, walk), f = unit_full_segments(d, n, walk);
            place(t0 + tid < n_tiles ? tile_of(t0 + tid) : 0u, d, n, f, full_base(f), 0u, false);
        }
    }
}

// the launch order of the backward blend's units (and the pass block: this is then the first kernel of the backward)
void issue_unit_order(const BwdPlan& p, BwdPassArgs* dst, const BwdPassArgs& v, hipStream_t s)
{
    if (!v.blend.unit_order) return;
    // slots of the longest list decide how many tiles a thread of the order kernel keeps in registers
    const uint32_t slots = TileGrid{(uint32_t)p.gx, (uint32_t)p.gy}.list_slots(0);
    if (slots <= (uint32_t)kOrderThreads)
        hipLaunchKernelGGL(unit_order_kernel<1>, dim3(kOrderLists), dim3(kOrderThreads), 0, s, dst, v);
    else if (slots <= 2u * (uint32_t)kOrderThreads)
        hipLaunchKernelGGL(unit_order_kernel<2>, dim3(kOrderLists), dim3(kOrderThreads), 0, s, dst, v);
    else
        hipLaunchKernelGGL(unit_order_kernel<8>, dim3(kOrderLists), dim3(kOrderThreads), 0, s, dst, v);
}

}  // namespace r3
