// row_table.h -- what the model-state units (densify.hip, mcmc.hip) share around their kernels: the
// plan's grid and workspace carving, and the table of tensors a move launch walks -- an entry per tensor of the caller's
// {src, dst, row_words, kind} array, a run of workgroups per entry.  Host and device.
#pragma once
#include "common.h"

namespace r3 {

constexpr int kPlanBlock = 256;          // a plan workgroup takes kPlanBlock Gaussians
constexpr long long kMaxP = 1LL << 30;   // 2 P destination rows are counted in int32
inline long long plan_blocks(long long P) { return (P + kPlanBlock - 1) / kPlanBlock; }
inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// Carves 16-byte aligned arrays off a workspace in the order they are taken.  From a null base it only counts: the size of
// a workspace is used() after the same takes, so the layout and its size cannot disagree.
struct Carver16 {
    char* base;
    size_t at = 0;
    template <typename T>
    T* take(size_t n)
    {
        T* r = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += round16(n * sizeof(T));
        return r;
    }
    size_t used() const { return at; }
};

struct RowEntry {
    const uint32_t* src;
    uint32_t* dst;
    long long chunk_begin;   // first workgroup of this tensor
    long long words;         // words the launch walks: rows * W
    int W;                   // words per row
    int kind;                // the unit's R3DGS_*_ kind
};

// The entry workgroup b belongs to: entries are few and in chunk order.
template <typename E>
__host__ __device__ __forceinline__ int entry_of(const E* e, int n, long long b)
{
    int ei = 0;
    while (ei + 1 < n && e[ei + 1].chunk_begin <= b) ei++;
    return ei;
}

// Validates tensors[0..n) and fills e[0..count): `rows` rows per tensor, chunk_words words per workgroup, kinds in
// [0, kind_max].  width_error(kind, row_words) and extra_error(src, dst) (may be empty) return the text of a refusal or
// NULL; a tensor of no words is skipped after the first.  Errors are "<what>: tensor <i><text>".  -> workgroups of the launch.
template <typename T, typename E>
long long fill_entries(const std::string& what, const T* tensors, int n, long long rows, int chunk_words, int kind_max,
                       const std::function<const char*(int, int)>& width_error,
                       const std::function<const char*(const void*, const void*)>& extra_error, E* e, int& count)
{
    long long chunks = 0;
    for (int i = 0; i < n; i++) {
        const T& x = tensors[i];
        const std::string where = what + ": tensor " + std::to_string(i);
        if (x.row_words < 0 || x.row_words > (1 << 20)) throw Error(where + ": row_words out of range");
        if (x.kind < 0 || x.kind > kind_max) throw Error(where + ": unknown kind");
        if (const char* text = width_error(x.kind, x.row_words)) throw Error(where + text);
        if (x.row_words == 0) continue;
        if (!x.src || !x.dst) throw Error(where + ": src or dst is NULL");
        if ((uintptr_t)x.src % 4 || (uintptr_t)x.dst % 4) throw Error(where + ": not 4-byte aligned");
        if (extra_error)
            if (const char* text = extra_error(x.src, x.dst)) throw Error(where + text);
        E& y = e[count++];
        y.src = static_cast<const uint32_t*>(x.src);
        y.dst = static_cast<uint32_t*>(x.dst);
        y.chunk_begin = chunks;
        y.words = rows * x.row_words;
        y.W = x.row_words;
        y.kind = x.kind;
        chunks += (y.words + chunk_words - 1) / chunk_words;
        if (chunks >= (1LL << 31)) throw Error(what + ": too many elements in one launch");
    }
    return chunks;
}

}  // namespace r3
