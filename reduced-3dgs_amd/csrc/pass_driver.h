// pass_driver.h -- what the extern "C" boundary (capi.hip) needs from the pass driver (pass_driver.hip): the calls it
// fills, the three drivers, and the library state its setters and queries reach.
#pragma once
#include <atomic>

#include "../../include/r3dgs_rasterizer.h"
#include "common.h"

namespace r3 {

// A switch of the library: on unless its environment variable says 0 (read at the first use), and settable through the C
// ABI afterwards.
struct Toggle {
    const char* env;
    std::atomic<int> v{-1};
    int get()
    {
        int x = v.load();
        if (x < 0) {
            x = env_int(env, 1, 0, 1);
            v.store(x);
        }
        return x;
    }
    int set(int on)   // on < 0: query only; returns the value before the call
    {
        const int before = get();
        if (on >= 0) v.store(on ? 1 : 0);
        return before;
    }
};
extern Toggle g_tight_rects, g_tile_order, g_bwd_segments, g_sh_cache, g_f64_chain;   // what each selects: pass_driver.hip

struct FwdCall {
    int P;
    const int* D;
    int M;
    const int *coeffsNum, *perBand, *cumSum;
    const float* background;
    int width, height;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp, *viewmatrix, *projmatrix, *cam_pos;
    float tan_fovx, tan_fovy;
    float* out_color;
    int* out_touched_pixels;
    float* out_transmittance;
    int* radii;
    int calculate_mean_transmittance, debug;
    hipStream_t stream;
    // raw-parameter entry (r3dgs_forward_params*): scales / rotations are the model's raw parameters, shs is features_dc
    // and shs_rest features_rest (common.h, behind FwdInputs)
    const float* shs_rest;
    int raw;
    // quantised entry (r3dgs_quantised_forward*): the model is `quant` (common.h, behind shs_rest); the five model pointers
    // above are NULL and the band tables are the ragged path's
    int quantised = 0;
    QuantInputs quant = {};
};

// r3dgs_backward and r3dgs_backward_params.  raw: scales / rotations are the model's raw parameters and dL_dscale / dL_drot
// their gradients, shs / dL_dsh are features_dc / its gradient, shs_rest / dL_dsh_rest features_rest / its gradient.
struct BwdCall {
    int P;
    const int* D;
    int M, R;
    const float* background;
    int width, height;
    const float *means3D, *shs, *colors_precomp, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp, *viewmatrix, *projmatrix, *campos;
    float tan_fovx, tan_fovy;
    const int* radii;
    PassBlobs blobs;
    const float* dL_dpix;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
    float lambda_sh_sparsity;
    int debug;
    hipStream_t stream;
    const float* shs_rest;
    float* dL_dsh_rest;
    int raw;
    // r3dgs_backward_absgrad / r3dgs_backward_params_absgrad: the pass also returns the abs columns (common.h AbsGradArgs);
    // absgrad == 0: the plain pass, the three fields behind it are not looked at
    int absgrad = 0;
    float* dL_dmean2D_abs = nullptr;
    float* abs_workspace = nullptr;
    size_t abs_workspace_floats = 0;
};

// the refusals of the *_absgrad entry points (looked at before anything else of the call)
inline void check_absgrad_args(int R, bool has_binning, const float* out, const float* workspace, size_t workspace_floats)
{
    if (!out) throw Error("absgrad: dL_dmean2D_abs is NULL");
    const size_t need = absgrad_workspace_floats((size_t)(R > 0 ? R : 1));
    if (has_binning && (!workspace || workspace_floats < need))
        throw Error("absgrad: the workspace holds " + std::to_string(workspace ? workspace_floats : 0) +
                    " floats, r3dgs_absgrad_workspace_floats(R) = " + std::to_string(need));
}

struct Allocators {   // the exact-size contract's callbacks
    r3dgs_alloc_fn geometry;
    void* geometry_user;
    r3dgs_alloc_fn binning;
    void* binning_user;
    r3dgs_alloc_fn image;
    void* image_user;
};
// Exact-size forward (the reference's contract): allocator callbacks, returns num_rendered.
int forward_exact(const Allocators& alloc, const FwdCall& c);
// Reserved forward: caller-provided blobs, no host wait.  Returns the pass ticket.
long long forward_reserved(const PassBlobs& blobs, int reserve, const FwdCall& c);
int backward_pass(const BwdCall& c);

int last_forward_pairs();              // r3dgs_forward_pairs(): of this thread's last exact-size forward
void set_forward_trains(int trains);   // r3dgs_forward_hint(): holds for this thread's forwards until set again

size_t cached_depth_temp(size_t P);    // the generic depth sort's temp-storage query, asked once per P
size_t geometry_blob_bytes(size_t P, size_t depth_temp, bool lean);

// The published PassInfo of a ticket, acquired; wait = 0: nullptr if the pass has not published yet.  Throws on what is
// no ticket or one whose ring slot was reused.
const volatile PassInfo* pass_info(long long ticket, int wait);

// the reservation advice (reserve_advice.h) over the PassInfo ring, for the current device
uint32_t reserve_hint(int P, int W, int H, const float* viewmatrix);
void reserve_forget_view(const float* viewmatrix);
void reserve_forget_all();
long long reserve_overflow_events(int* last_num_rendered, int* last_reserve);

// the host preamble of the replay passes (`what`: the entry point's name, for the message)
inline void check_replay_dims(const char* what, int P, int R, int width, int height)
{
    if (width < 1 || height < 1 || P < 0 || R < 0)
        throw Error(std::string(what) + ": need width, height >= 1 and P, R >= 0, got P = " + std::to_string(P) + ", R = " +
                    std::to_string(R) + ", " + std::to_string(width) + "x" + std::to_string(height));
}
inline TileGrid replay_grid(const char* what, int width, int height)   // a walk launches four workgroups per tile
{
    const TileGrid grid = grid_of(width, height);
    if (grid.n() * 4 > 0x7fffffffull) throw Error(std::string(what) + ": the image has too many tiles for one launch");
    return grid;
}

// the three state blobs of a call that walks, carved (arithmetic only: nothing is read here)
inline PassStates replay_states(const char* what, int P, int R, int width, int height, const PassBlobs& blobs)
{
    if (!blobs.geom || !blobs.binning || !blobs.image) throw Error(std::string(what) + ": state buffers must not be NULL");
    return carve_pass(P, (uint32_t)R, width, height, blobs, 0);
}
// What a replay backward does (DESIGN.md "Replay passes", the host contract), in the order the cases are tried: every output
// has P rows, so P == 0 leaves nothing to write; without pairs or without an upstream gradient the outputs are zeros and the
// blobs are not read; a walk nobody reads is not launched.
enum class ReplayPlan { Nothing, ZeroOutputs, Walk };
inline ReplayPlan replay_bwd_plan(int P, int R, bool has_upstream, bool any_output)
{
    if (P == 0) return ReplayPlan::Nothing;
    if (R == 0 || !has_upstream) return ReplayPlan::ZeroOutputs;
    return any_output ? ReplayPlan::Walk : ReplayPlan::Nothing;
}

void profile_enable(int on);
void profile_read(double* total_ms, int* launches);

}  // namespace r3
