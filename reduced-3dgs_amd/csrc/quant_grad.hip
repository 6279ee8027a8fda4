// quant_grad.hip -- r3dgs_quantised_codebook_grad: the adjoint of the codebook lookup (include/r3dgs_quantised.h).
//
// Per Gaussian, up to 56 gradient floats (quant_math.h quant_grad_slot) are summed into the 20 x 256 centres their ids name.
// No float or double atomics anywhere; every centre's sum is accumulated in double in an order that (P, the ids) fix, and
// rounded to float once, so two calls give the same bits.
//
//   quantised_codebook_grad_kernel   one wave per group of consecutive chunks, one Gaussian per lane, 64 at a time.  In slot
//       trip s every lane holds (id, value) for the same book.  The lanes that share an id find each other with eight
//       ballots over the id's bits; a lane's rank among its peers is the popcount below it.  In round r the rank-r lanes add
//       into the wave's private double tables in LDS: no two lanes touch one entry within a round, and a barrier orders the
//       rounds.  The order of a centre's sum is therefore (64-batch, slot, lane).  The tables go to the workspace.
//   quantised_codebook_grad_finish   one thread per centre adds the groups' partials in group order and rounds.
//
// Every gradient element and id byte is read once: a lane walks its own rows, so a trip's loads are strided, but the lines
// they touch are used up by the following trips out of the cache.
#include "common.h"
#include "quant_math.h"

namespace r3 {

namespace {

constexpr int kTable = kQuantBooks * kQuantCentres;   // 5120 doubles = 40 KB: four waves per CU

struct QuantGradIn {
    const float* t[kQuantGradTensors];   // indexed by QuantGradTensor; NULL counts as zeros
};

struct Trip {   // what a lane brings to one slot trip
    bool own;
    unsigned id;
    int book;
    float value;
};

__device__ inline const float* grad_tensor(const QuantGradIn& g, int which)
{
    const float* p = g.t[kGradDc];
    p = which == kGradRest ? g.t[kGradRest] : p;
    p = which == kGradOpacity ? g.t[kGradOpacity] : p;
    p = which == kGradScaling ? g.t[kGradScaling] : p;
    p = which == kGradRotation ? g.t[kGradRotation] : p;
    return p;
}

__global__ __launch_bounds__(64) void quantised_codebook_grad_kernel(int P, int chunks_per_group, const int* __restrict__ coeffs,
                                                                     const int* __restrict__ perband,
                                                                     const int* __restrict__ cumsum,
                                                                     const uint8_t* __restrict__ geom_ids,
                                                                     const uint8_t* __restrict__ sh_ids, QuantGradIn g,
                                                                     double* __restrict__ partials)
{
    __shared__ double table[kTable];
    const int lane = threadIdx.x;
    for (int k = lane; k < kTable; k += 64) table[k] = 0.0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long span = (long long)chunks_per_group * kQuantGradChunk;
    const long long first = (long long)blockIdx.x * span;
    const long long last = first + span < (long long)P ? first + span : (long long)P;
    for (long long base = first; base < last; base += 64) {
        const long long i = base + lane;
        const bool live = i < last;
        int deg = 0;
        const long long sh_off = live ? 3LL * quant_ragged_offset((int)i, coeffs, perband, cumsum, &deg) : 0;
        // the loads of trip s + 1 are in flight while trip s is ranked and added
        auto fetch = [&](int s) {
            Trip t = {false, 0u, 0, 0.0f};
            QuantGradSlot slot;
            if (live && s < kQuantSlots && quant_grad_slot(s, i, deg, sh_off, geom_ids, sh_ids, &slot)) {
                const float* src = grad_tensor(g, slot.tensor);
                if (src != nullptr) {
                    t.own = true;
                    t.id = *slot.id;
                    t.book = slot.book;
                    t.value = src[slot.elem];
                }
            }
            return t;
        };
        Trip next = fetch(0);
        for (int s = 0; s < kQuantSlots; s++) {
            const Trip t = next;
            next = fetch(s + 1);
            const unsigned long long active = __ballot(t.own);
            if (active == 0) continue;   // (wave-uniform: the barriers below stay convergent)
            unsigned long long peers = active;
            for (int b = 0; b < 8; b++) {
                const bool bit = (t.id >> b) & 1u;
                const unsigned long long set = __ballot(bit);
                peers &= bit ? set : ~set;
            }
            const int rank = __popcll(peers & below);
            const int entry = t.book * kQuantCentres + (int)t.id;   // (0 for a lane that does not take part)
            const double v = (double)t.value;
            for (int r = 0; __ballot(t.own && rank >= r) != 0; r++) {
                if (t.own && rank == r) table[entry] += v;
                __syncthreads();
            }
        }
    }
    double* out = partials + (long long)blockIdx.x * kTable;
    for (int k = lane; k < kTable; k += 64) out[k] = table[k];
}

__global__ __launch_bounds__(256) void quantised_codebook_grad_finish(int groups, const double* __restrict__ partials,
                                                                      float* __restrict__ dL_dcodebooks)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= kTable) return;
    double sum = 0.0;   // a centre nobody names stays +0.0
    for (int grp = 0; grp < groups; grp++) sum += partials[(long long)grp * kTable + k];
    dL_dcodebooks[k] = (float)sum;
}

}  // namespace

size_t quantised_codebook_grad_workspace_bytes(int P)
{
    return P <= 0 ? 0 : (size_t)quant_grad_groups(P) * kTable * sizeof(double);
}

void launch_quantised_codebook_grad(int P, const int* coeffs, const int* perband, const int* cumsum, const unsigned char* geom_ids,
                                    const unsigned char* sh_ids, const float* dL_dfeatures_dc, const float* dL_dfeatures_rest,
                                    const float* dL_dopacity, const float* dL_dscaling, const float* dL_drotation,
                                    float* dL_dcodebooks, void* workspace, hipStream_t s)
{
    const int groups = P <= 0 ? 0 : quant_grad_groups(P);
    double* partials = static_cast<double*>(workspace);
    if (groups) {
        QuantGradIn g;
        g.t[kGradDc] = dL_dfeatures_dc;
        g.t[kGradRest] = dL_dfeatures_rest;
        g.t[kGradOpacity] = dL_dopacity;
        g.t[kGradScaling] = dL_dscaling;
        g.t[kGradRotation] = dL_drotation;
        hipLaunchKernelGGL(quantised_codebook_grad_kernel, dim3(groups), dim3(64), 0, s, P, quant_grad_chunks_per_group(P), coeffs,
                           perband, cumsum, geom_ids, sh_ids, g, partials);
    }
    hipLaunchKernelGGL(quantised_codebook_grad_finish, dim3((kTable + 255) / 256), dim3(256), 0, s, groups, partials, dL_dcodebooks);
}

}  // namespace r3
