// aux_bwd_stage.h -- what the units with an aux-style backward share (aux_bwd.hip, distortion.hip, feature_maps.hip):
//   * the slab rows a pixel pass writes (aux_bwd_pixel_kernel, dist_bwd_pixel_kernel): 32-byte rows of seven wave sums at
//     slab[(list slot * 4 + quadrant) * 8], zero rows for an entry nobody blended and for the slots behind the walk;
//   * the ends of a per-Gaussian kernel: the zero gradient and the six guarded stores;
//   * the opening of a backward entry point (replay_bwd_open) and the fill of a per-Gaussian kernel's arguments;
//   * the host side of aux_bwd.hip's second stage (defined there): the workspace layout, the zero fill of a call with
//     nothing to walk, and the three launches behind the pixel pass -- keys, the stable sort (pair_sort.h), the per-Gaussian
//     sum in double and chain.
#pragma once
#include <optional>

#include "aux_math.h"
#include "common.h"
#include "pair_sort.h"
#include "pass_driver.h"
#include "replay_walk.h"

namespace r3 {

// ---- slab rows (two float4 per row) -------------------------------------------------------------------------------------
__device__ __forceinline__ size_t slab_row(const WalkSpan& sp, uint32_t k, int quad)   // of list position k, in float4
{
    return ((size_t)(sp.first + k) * kAuxQuads + (size_t)quad) * 2;
}

// the slots behind the walk: zero rows
__device__ __forceinline__ void slab_zero_behind(R3_GLOBAL float4* rows, const WalkSpan& sp, int quad, int lane)
{
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t k = sp.len + (uint32_t)lane; k < sp.list_len; k += kWalkChunk) {
        const size_t row = slab_row(sp, k, quad);
        rows[row] = zero4;
        rows[row + 1] = zero4;
    }
}

// the seven sums of entry j over the wave, parked in the slab's order (aux_math.h aux_row_of): sx, sy, sxx, sxy, syy, sm, sz
__device__ __forceinline__ void slab_park_sums(float4 (*s_out)[2], int j, int lane, const SplatSums& sg)
{
    const float r0 = wave_sum_ror(sg.sx), r1 = wave_sum_ror(sg.sy), r2 = wave_sum_ror(sg.sxx);
    const float r3 = wave_sum_ror(sg.sxy), r4 = wave_sum_ror(sg.syy), r5 = wave_sum_ror(sg.sm);
    const float r6 = wave_sum_ror(sg.r);
    if (lane == 0) {
        s_out[j][0] = make_float4(r0, r1, r2, r3);
        s_out[j][1] = make_float4(r4, r5, r6, 0.f);
    }
}

// lane j stores the row of entry j of the chunk at cbase: the parked sums, or zeros for an entry no lane blended
__device__ __forceinline__ void slab_store_chunk(R3_GLOBAL float4* rows, const float4 (*s_out)[2], const WalkSpan& sp, int quad,
                                                 uint32_t cbase, int lane, unsigned long long contributed)
{
    if (cbase + (uint32_t)lane < sp.len) {
        const bool have = (contributed >> lane) & 1ull;
        const size_t row = slab_row(sp, cbase + (uint32_t)lane, quad);
        float4 o0 = s_out[lane][0], o1 = s_out[lane][1];
        if (!have) o0 = o1 = make_float4(0.f, 0.f, 0.f, 0.f);
        rows[row] = o0;
        rows[row + 1] = o1;
    }
}

// what the per-Gaussian chain reads besides the state blobs, and the six outputs (any of them nullptr: not written)
struct AuxBwdGeom {
    const float *viewmatrix, *projmatrix;
    float tan_fovx, tan_fovy;
    const float *means3D, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp;
    const int* radii;
    float *dL_dmeans2D, *dL_dmeans3D, *dL_dopacity, *dL_dscales, *dL_drotations, *dL_dcov3D;
    // the _screen entry points' two: dL_dconic [P,4] (A, B, unused, C) and dL_dz [P], for a camera pass behind the call
    float *dL_dconic = nullptr, *dL_dz = nullptr;
    bool screen_output() const { return dL_dconic || dL_dz; }
    // what the chain behind the screen-space sums is run for (dL_dmeans2D needs none of it)
    bool model_output() const { return dL_dmeans3D || dL_dopacity || dL_dscales || dL_drotations || dL_dcov3D; }
    bool any_output() const { return dL_dmeans2D || model_output() || screen_output(); }
};

// ---- the per-Gaussian kernels' shared ends --------------------------------------------------------------------------------
// (A: a kernel's argument struct with the six output pointers.  The middle -- camera and parameter loads, aux_math.h
// aux_bwd_chain -- stays written out in aux_bwd_gauss_kernel and feat_bwd_gauss_kernel: behind a function boundary the
// compiler orders the operands of the chain's commutative fp32 operations differently, contracts the other product of a
// sum of two into the FMA, and the gradients' last bits move.)
__device__ __forceinline__ void gauss_grad_clear(AuxGaussGrad& o)
{
    o.mean2D[0] = o.mean2D[1] = o.opacity = 0.f;
    for (int k = 0; k < 3; k++) o.mean3D[k] = o.scale[k] = 0.f;
    for (int k = 0; k < 4; k++) o.rot[k] = 0.f;
    for (int k = 0; k < 6; k++) o.cov6[k] = 0.f;
}

// row i of every output that is asked for
template <class A>
__device__ __forceinline__ void gauss_grad_store(const A& a, uint32_t i, const AuxGaussGrad& o)
{
    if (a.dL_dmeans2D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dmeans2D) + 3 * (size_t)i;
        d[0] = o.mean2D[0];
        d[1] = o.mean2D[1];
        d[2] = 0.f;
    }
    if (a.dL_dmeans3D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dmeans3D) + 3 * (size_t)i;
        for (int k = 0; k < 3; k++) d[k] = o.mean3D[k];
    }
    if (a.dL_dopacity) global_ptr(a.dL_dopacity)[i] = o.opacity;
    if (a.dL_dscales) {
        R3_GLOBAL float* d = global_ptr(a.dL_dscales) + 3 * (size_t)i;
        for (int k = 0; k < 3; k++) d[k] = o.scale[k];
    }
    if (a.dL_drotations) {
        R3_GLOBAL float* d = global_ptr(a.dL_drotations) + 4 * (size_t)i;
        for (int k = 0; k < 4; k++) d[k] = o.rot[k];
    }
    if (a.dL_dcov3D) {
        R3_GLOBAL float* d = global_ptr(a.dL_dcov3D) + 6 * (size_t)i;
        for (int k = 0; k < 6; k++) d[k] = o.cov6[k];
    }
}

// ---- the host side, defined in aux_bwd.hip ------------------------------------------------------------------------------
// bytes of the workspace for a pair capacity R > 0 (asks rocPRIM once per R: call it outside a capture first)
size_t aux_bwd_workspace_bytes(size_t R);
// the slab inside a workspace: [R][4 quadrants][8 floats], every (slot < num_pairs, quadrant) row written by the pixel pass
float* aux_bwd_slab(char* workspace, size_t R);
// P rows of zeros in every output that is asked for
void aux_bwd_zero_outputs(int P, const AuxBwdGeom& g, hipStream_t s);
// the pointer checks of a call that walks (`what`: the entry point's name, for the message)
void aux_bwd_check_geom(const char* what, const AuxBwdGeom& g);
// The opening of a backward entry point, by the plan of pass_driver.h replay_bwd_plan: nullopt when the call is complete
// (nothing to do, or the outputs -- `rows_out`, P rows of `row_floats`, is a unit's output beside g's six -- were zero-filled),
// else the carved state and the grid of a call that walks.  check_dims(what) and check_inputs() are the unit's own refusals:
// the first of all, and behind the NULL checks on the blobs and the workspace.
struct ReplayBwdWalk {
    PassStates st;
    TileGrid grid;
};
template <class Dims, class Inputs>
std::optional<ReplayBwdWalk> replay_bwd_open(const char* what, int P, int R, int width, int height, const PassBlobs& blobs,
                                             bool has_upstream, const AuxBwdGeom& g, float* rows_out, size_t row_floats,
                                             const char* workspace, hipStream_t s, Dims check_dims, Inputs check_inputs)
{
    check_dims(what);
    const ReplayPlan plan = replay_bwd_plan(P, R, has_upstream, g.any_output() || rows_out);
    if (plan == ReplayPlan::ZeroOutputs) {
        if (rows_out) R3_HIP(hipMemsetAsync(rows_out, 0, sizeof(float) * row_floats * (size_t)P, s));
        aux_bwd_zero_outputs(P, g, s);
    }
    if (plan != ReplayPlan::Walk) return std::nullopt;
    const PassStates st = replay_states(what, P, R, width, height, blobs);
    if (!workspace) throw Error(std::string(what) + ": the workspace must not be NULL");
    check_inputs();
    return ReplayBwdWalk{st, replay_grid(what, width, height)};
}
// The arguments of a per-Gaussian kernel (A: AuxGaussArgs, FeatGaussArgs) but for its slab and what else is the unit's own.
template <class A>
A gauss_args_of(const PassStates& st, const PairSortWork& sort, int P, int R, int width, int height, const AuxBwdGeom& in)
{
    A g = {};
    g.rec = st.geom.rec;
    g.radii = in.radii;
    g.tiles = st.geom.tiles;
    g.keys = sort.keys_out;
    g.slots = sort.slots_out;
    g.view = in.viewmatrix;
    g.proj = in.projmatrix;
    g.means3D = in.means3D;
    g.scales = in.scales;
    g.rotations = in.rotations;
    g.cov3D_precomp = in.cov3D_precomp;
    g.tan_fovx = in.tan_fovx;
    g.tan_fovy = in.tan_fovy;
    g.scale_modifier = in.scale_modifier;
    g.W = width;
    g.H = height;
    g.P = (uint32_t)P;
    g.R = (uint32_t)R;
    g.dL_dmeans2D = in.dL_dmeans2D;
    g.dL_dmeans3D = in.dL_dmeans3D;
    g.dL_dopacity = in.dL_dopacity;
    g.dL_dscales = in.dL_dscales;
    g.dL_drotations = in.dL_drotations;
    g.dL_dcov3D = in.dL_dcov3D;
    return g;
}
// keys, sort, per-Gaussian sum and chain over a slab the pixel pass has been launched on, on the same stream
void aux_bwd_second_stage(const PassStates& st, int P, int R, int width, int height, const AuxBwdGeom& g, char* workspace,
                          hipStream_t s);
// The per-Gaussian sum and chain of a call that asks for g.dL_dconic / g.dL_dz (the _screen entry points), over sorted keys
// and a slab of `rows_per_slot` 32-byte rows per list slot laid out as the aux slab's: the six outputs as the unit's own
// per-Gaussian kernel writes them, bit for bit, and the two screen-space ones.  With no model output asked for
// (!g.model_output()) the chain behind the screen-space sums is skipped and of the model only g.radii is read.
void launch_screen_gauss(const char* what, const PassStates& st, const PairSortWork& sort, int P, int R, int width, int height,
                         const AuxBwdGeom& g, const float* slab, uint32_t rows_per_slot, hipStream_t s);

}  // namespace r3
