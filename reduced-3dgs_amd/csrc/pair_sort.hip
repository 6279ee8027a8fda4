// pair_sort.hip -- (Gaussian id, list slot) pairs and their stable sort by id (pair_sort.h), gfx950.
#include <algorithm>
#include <cstring>   // (rocPRIM's texture iterator calls memset without including it)
#include <map>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "pair_sort.h"

namespace r3 {

namespace {

// (Gaussian id, list slot) per slot of the pair capacity
__global__ __launch_bounds__(256) void pair_keys_kernel(const GeomHeader* hdr, const uint32_t* point_list, uint32_t P, uint32_t R,
                                                        uint32_t* keys, uint32_t* slots)
{
    const uint32_t num_pairs = min(global_ptr(hdr)->num_pairs, R);
    for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < R; e += gridDim.x * 256u) {
        uint32_t key = 0xffffffffu;
        if (e < num_pairs) {
            const uint32_t id = global_ptr(point_list)[e];
            if (id < P) key = id;
        }
        global_ptr(keys)[e] = key;
        global_ptr(slots)[e] = e;
    }
}

}  // namespace

size_t pair_sort_temp_bytes(size_t R)
{
    static std::mutex mu;
    static std::map<size_t, size_t> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find(R);
    if (it != known.end()) return it->second;
    size_t bytes = 0;
    R3_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     R, 0, 32, (hipStream_t)0));
    known[R] = bytes;
    return bytes;
}

void launch_pair_sort(const char* what, const PassStates& st, int P, int R, const PairSortWork& w, hipStream_t s)
{
    const uint32_t key_blocks = (uint32_t)std::min<size_t>(((size_t)R + 255) / 256, 4096);
    hipLaunchKernelGGL(pair_keys_kernel, dim3(key_blocks), dim3(256), 0, s, st.geom.header, st.bin.point_list, (uint32_t)P,
                       (uint32_t)R, w.keys_in, w.slots_in);
    check_launch((std::string(what) + ", keys").c_str(), s, false);
    size_t temp = w.temp_bytes;
    R3_HIP(rocprim::radix_sort_pairs(w.temp, temp, w.keys_in, w.keys_out, w.slots_in, w.slots_out, (size_t)R, 0, 32, s));
}

}  // namespace r3
