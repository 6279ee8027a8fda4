// unit_order.h -- the launch order of the backward blend's units, as a rule: what a unit word holds, where the lists and their
// trailers lie, and how many segments a tile is walked in, what each weighs and which class that weight falls into.
//
// A UNIT is what one workgroup of the backward blend walks: a tile, or -- for a tile whose list the pass splits (common.h) --
// one segment of its list.  The order is kOrderLists lists (common.h TileGrid), each sorted by decreasing weight class.
// Four parties read this header and nothing else about the order: unit_order.hip (the counting sort that writes it),
// blend.hip (blend_bwd_kernel decodes its unit), pass_driver.hip (sizes the array) and capi.hip (exports it);
// tests/hostcheck_unit_order replays the same functions serially on the CPU.  Integer arithmetic, and the one fp32 multiply of the class.
#pragma once
#include "common.h"

namespace r3 {

constexpr int kOrderThreads = 1024, kOrderClasses = 1024;
constexpr uint32_t kClassBits = 10;   // a class in the packed classes a thread keeps between counting and placement
constexpr uint32_t kCached = 3u;      // classes of a tile's first partial segments kept that way
constexpr uint32_t kWalks = 4;        // segment lengths a pass may walk: S, 2 S, 4 S, 8 S (the first whose units fit the launch)
static_assert(kOrderClasses <= (1 << kClassBits) && kCached * kClassBits <= 32, "the cached classes are packed into one word");

R3_HD uint32_t umin_(uint32_t a, uint32_t b) { return a < b ? a : b; }
R3_HD uint32_t umax_(uint32_t a, uint32_t b) { return a > b ? a : b; }

// ---- the unit word: tile | segment << kUnitTileBits | segments << (kUnitTileBits + kUnitSegBits) ---------------------------
constexpr uint32_t kUnitSegBits = 6;
static_assert(kUnitTileBits + 2 * kUnitSegBits <= 32, "a unit is one 32-bit word");
static_assert(kBwdSegMax < (1 << kUnitSegBits), "the segment count of a tile (kBwdSegMax at most) must fit its field");
struct Unit {
    uint32_t tile, segment, segments;
};
R3_HD uint32_t unit_pack(uint32_t tile, uint32_t segment, uint32_t segments)
{
    return tile | (segment << kUnitTileBits) | (segments << (kUnitTileBits + kUnitSegBits));
}
R3_HD Unit unit_unpack(uint32_t u)
{
    return Unit{u & ((1u << kUnitTileBits) - 1u), (u >> kUnitTileBits) & ((1u << kUnitSegBits) - 1u),
                u >> (kUnitTileBits + kUnitSegBits)};
}

// ---- list addressing: word offsets into the order array of a pass whose lists hold `units_cap` slots together -------------
// [kOrderLists lists of unit_list_cap slots][kOrderLists trailers {units of the list, log2 of the segment length they walk}]
// (common.h unit_order_words: what BinState::carve and the export take)
R3_HD uint32_t unit_list_cap(uint32_t units_cap) { return units_cap / kOrderLists; }
R3_HD uint32_t unit_list_base(uint32_t units_cap, uint32_t g) { return g * unit_list_cap(units_cap); }
R3_HD uint32_t unit_trailer(uint32_t units_cap, uint32_t g) { return units_cap + kUnitTrailerWords * g; }
static_assert(kUnitTrailerWords == 2, "a trailer is {units, walk_log2}");   // the array's size: common.h unit_order_words
// the trailer of list g in the array at `order`: behind the lists, then to the list's pair (two pointer steps, as the kernels
// have always formed it: folded into one 32-bit offset the kernels' scalar code and its schedule change)
template <class W>
R3_HD W* unit_trailer_at(W* order, uint32_t units_cap, uint32_t g)
{
    return order + unit_trailer(units_cap, 0u) + unit_trailer(0u, g);
}

// ---- the per-tile rule ----------------------------------------------------------------------------------------------------
// `d`: the deepest contributor of each of the tile's four quadrants (ImageState::quad_depth); `walk`: log2 of the segment
// length the pass walks (0: whole tiles); `thr`: the list length from which the forward left checkpoints.

// segments of 2^walk entries the backward walks a tile in: 1 unless the forward left checkpoints for it (list length)
// and it is deeper than one segment
R3_HD uint32_t unit_segments(uint32_t list_len, uint32_t deepest, uint32_t thr, uint32_t walk)
{
    if (list_len < thr || deepest <= (1u << walk)) return 1u;
    return umin_((deepest + (1u << walk) - 1u) >> walk, (uint32_t)kBwdSegMax);
}
// units of a tile: its segments, or none for a tile nothing contributed to
R3_HD uint32_t unit_count(const uint4& d, uint32_t list_len, uint32_t thr, uint32_t walk)
{
    if (d.x + d.y + d.z + d.w == 0u) return 0u;
    return walk ? unit_segments(list_len, umax_(umax_(d.x, d.y), umax_(d.z, d.w)), thr, walk) : 1u;
}
// Leading segments of a tile of n units that all four quadrants walk in full: each weighs 4 x the segment length.
// (A capped tile's last segment takes the rest: not "full".)
R3_HD uint32_t unit_full_segments(const uint4& d, uint32_t n, uint32_t walk)
{
    if (n <= 1u) return 0u;
    const uint32_t f = umin_(umin_(d.x, d.y), umin_(d.z, d.w)) >> walk;
    return umin_(f, n == (uint32_t)kBwdSegMax ? n - 1u : n);
}
// entries segment `s` of `n` visits in the four quadrants whose deepest contributors are d
R3_HD uint32_t unit_weight(const uint4& d, uint32_t s, uint32_t n, uint32_t walk)
{
    if (n == 1u) return d.x + d.y + d.z + d.w;
    const uint32_t lo = s << walk, hi = s + 1u < n ? lo + (1u << walk) : 0xFFFFFFFFu;
    auto part = [&](uint32_t q) { return umin_(umax_(q, lo), hi) - lo; };
    return part(d.x) + part(d.y) + part(d.z) + part(d.w);
}

// ---- classes: a counting sort over kOrderClasses weight classes, class 0 = the heaviest ------------------------------------
// The heaviest unit of a pass that splits, known without looking: a whole tile is shorter than `thr` entries (or it would be
// split) and no deeper than its list, a segment weighs at most 4 x its length -- only the last segment of a tile capped at
// kBwdSegMax can be heavier, and lands in the heaviest class.
R3_HD uint32_t unit_heaviest_bound(uint32_t thr, uint32_t walk) { return umax_(4u << walk, 4u * umin_(thr, 1u << 20)); }
R3_HD float unit_class_scale(uint32_t heaviest) { return (float)(kOrderClasses - 1) / (float)umax_(heaviest, 1u); }
R3_HD uint32_t unit_class(uint32_t weight, float scale)
{
    return (uint32_t)(kOrderClasses - 1) - umin_((uint32_t)((float)weight * scale), (uint32_t)(kOrderClasses - 1));
}

// ---- the walk progression: S, 2 S, 4 S, 8 S, then whole tiles (0) ---------------------------------------------------------
// A list whose units do not fit what it may launch (bwd_list_fit) counts again with the next length; whole tiles always fit.
R3_HD bool unit_walk_fits(uint32_t walk, uint32_t units, uint32_t fit) { return walk == 0u || units <= fit; }
R3_HD uint32_t unit_next_walk(uint32_t walk, uint32_t seg_log2) { return walk + 1u < seg_log2 + kWalks ? walk + 1u : 0u; }

}  // namespace r3
