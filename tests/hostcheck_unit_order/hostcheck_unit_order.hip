// Host shim of the backward blend's unit order (reduced-3dgs_amd/csrc/unit_order.h): a serial replay of what
// unit_order.hip's workgroup of one list computes, from the header's functions and common.h's TileGrid alone, and the pack /
// unpack of a unit word.  Loaded with ctypes by tests/test_unit_order_cpu.py and tests/test_gpu_parity.py.
#include <vector>

#include "../../reduced-3dgs_amd/csrc/unit_order.h"

using namespace r3;

extern "C" {

unsigned hu_pack(unsigned tile, unsigned segment, unsigned segments) { return unit_pack(tile, segment, segments); }
void hu_unpack(unsigned word, unsigned* out)
{
    const Unit u = unit_unpack(word);
    out[0] = u.tile;
    out[1] = u.segment;
    out[2] = u.segments;
}
// {kOrderLists, kOrderClasses, kWalks, kBwdSegMax, kUnitTileBits, kUnitSegBits}
void hu_constants(int* out)
{
    out[0] = (int)kOrderLists;
    out[1] = kOrderClasses;
    out[2] = (int)kWalks;
    out[3] = kBwdSegMax;
    out[4] = (int)kUnitTileBits;
    out[5] = (int)kUnitSegBits;
}
// words of the order array of a pass of `units_cap` slots; info = {list capacity, base of list g, trailer of list g}
unsigned hu_addressing(unsigned units_cap, unsigned g, unsigned* info)
{
    info[0] = unit_list_cap(units_cap);
    info[1] = unit_list_base(units_cap, g);
    info[2] = unit_trailer(units_cap, g);
    return unit_order_words(units_cap);
}

// The order of list `list` of a gx x gy tile grid: quad_depth[tiles][4], ranges[tiles][2], the pass's pair count, the
// forward's segment length (log2; 0: no checkpoints) and list-length threshold.  Writes the list's unit words in class order
// (ties inside a class in slot order, a tile's segments ascending), each unit's weight and class, per tile of the list its
// full segments (full[tiles]), and the trailer {units, walk_log2}.  As in the kernel a tile's full segments (unit_full_segments)
// go to the class of 4 x the segment length without their weight being looked at; the caller checks that this is their class.
// Returns the unit count, or -1 if `cap` words do not hold them.
int hu_replay(int gx, int gy, int list, const unsigned* quad_depth, const unsigned* ranges, unsigned num_pairs, unsigned seg_log2,
              unsigned thr, unsigned* words, unsigned* weights, unsigned* classes, unsigned* full, int cap, unsigned* trailer)
{
    const TileGrid grid{(uint32_t)gx, (uint32_t)gy};
    const uint32_t slots = grid.list_slots((uint32_t)list), fit = bwd_list_fit(num_pairs, grid);
    if (seg_log2 == 0u) thr = 0xFFFFFFFFu;
    std::vector<uint4> d(slots, make_uint4(0u, 0u, 0u, 0u));
    std::vector<uint32_t> len(slots, 0u), tile(slots, 0xFFFFFFFFu);
    for (uint32_t j = 0; j < slots; j++) {
        tile[j] = grid.list_tile((uint32_t)list, j);
        if (tile[j] == 0xFFFFFFFFu) continue;
        const unsigned* q = quad_depth + 4 * (size_t)tile[j];
        d[j] = make_uint4(q[0], q[1], q[2], q[3]);
        len[j] = ranges[2 * (size_t)tile[j] + 1] - ranges[2 * (size_t)tile[j]];
    }
    uint32_t walk = seg_log2;
    float scale = 0.f;
    std::vector<uint32_t> count;
    auto klass = [&](uint32_t j, uint32_t k, uint32_t n, uint32_t f) {   // full segments: one class, whatever they weigh
        return k < f ? unit_class(4u << walk, scale) : unit_class(unit_weight(d[j], k, n, walk), scale);
    };
    for (;;) {
        uint32_t heaviest = 0u;
        if (walk)
            heaviest = unit_heaviest_bound(thr, walk);
        else
            for (uint32_t j = 0; j < slots; j++) heaviest = umax_(heaviest, d[j].x + d[j].y + d[j].z + d[j].w);
        scale = unit_class_scale(heaviest);
        count.assign(kOrderClasses + 1, 0u);   // count[c + 1]: units of class c, then the first slot of class c + 1
        for (uint32_t j = 0; j < slots; j++) {
            const uint32_t n = unit_count(d[j], len[j], thr, walk), f = unit_full_segments(d[j], n, walk);
            for (uint32_t k = 0; k < n; k++) count[klass(j, k, n, f) + 1]++;
        }
        for (int c = 0; c < kOrderClasses; c++) count[c + 1] += count[c];
        if (unit_walk_fits(walk, count[kOrderClasses], fit)) break;
        walk = unit_next_walk(walk, seg_log2);
    }
    const uint32_t total = count[kOrderClasses];
    trailer[0] = total;
    trailer[1] = walk;
    if ((int)total > cap) return -1;
    for (uint32_t j = 0; j < slots; j++) {
        const uint32_t n = unit_count(d[j], len[j], thr, walk), f = unit_full_segments(d[j], n, walk);
        if (tile[j] != 0xFFFFFFFFu) full[tile[j]] = f;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t w = unit_weight(d[j], k, n, walk), c = klass(j, k, n, f), at = count[c]++;
            words[at] = unit_pack(tile[j], k, n);
            weights[at] = w;
            classes[at] = c;
        }
    }
    return (int)total;
}

}  // extern "C"
