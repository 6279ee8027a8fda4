// pair_sort.h -- the second stage's regrouping, for the replay passes that park rows per list slot (aux_bwd.hip,
// feature_maps.hip, importance.hip): (Gaussian id, list slot) per slot of the pair capacity, stably sorted by id, so that
// a Gaussian finds its rows as one run of the sorted keys, its slots ascending.  Defined in pair_sort.hip (integer code: no
// rounding depends on that unit's flags).
#pragma once
#include "common.h"

namespace r3 {

// rocPRIM's temp storage for R pairs.  Asked once per R: the query is host work, and a captured call must not repeat it
// (call a *_workspace_bytes entry outside a capture first).
size_t pair_sort_temp_bytes(size_t R);

// the tail of a unit's workspace, taken after the unit's own slabs: the (id, slot) arrays before and after the sort, the
// temp storage
struct PairSortWork {
    uint32_t *keys_in, *slots_in, *keys_out, *slots_out;
    char* temp;
    size_t temp_bytes;
    static PairSortWork carve(Carver& c, size_t R, size_t temp_bytes)
    {
        PairSortWork w;
        w.keys_in = c.take<uint32_t>(R);
        w.slots_in = c.take<uint32_t>(R);
        w.keys_out = c.take<uint32_t>(R);
        w.slots_out = c.take<uint32_t>(R);
        w.temp = c.take<char>(temp_bytes);
        w.temp_bytes = temp_bytes;
        return w;
    }
};

// Two launches on `s`: the keys (the key of a slot at or beyond the header's num_pairs, or of an id outside the model, is
// 0xffffffff), then the stable sort into keys_out / slots_out.  `what`: the pass's name, for a launch error.
void launch_pair_sort(const char* what, const PassStates& st, int P, int R, const PairSortWork& w, hipStream_t s);

// the first slot of the sorted keys that is not below i: where the run of Gaussian i starts, if it has one
__device__ __forceinline__ uint32_t run_begin(const uint32_t* keys, uint32_t R, uint32_t i)
{
    uint32_t lo = 0u, hi = R;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (global_ptr(keys)[mid] < i)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

// the run of Gaussian i in the sorted keys: [lo, lo + count).  (A kernel that reads one row set per pair may walk the run
// from run_begin() itself and count as it goes: aux_bwd_gauss_kernel, where the second pass over the keys costs 5 %.)
__device__ __forceinline__ uint32_t run_of(const uint32_t* keys, uint32_t R, uint32_t i, uint32_t* count)
{
    const uint32_t lo = run_begin(keys, R, i);
    uint32_t j = lo;
    while (j < R && global_ptr(keys)[j] == i) j++;
    *count = j - lo;
    return lo;
}

}  // namespace r3
