// aux_bwd_stage.h -- the second stage of aux_bwd.hip, for the units whose pixel pass writes the same slab (distortion.hip):
// the workspace layout, the zero-fill of a call with nothing to walk, and the three launches behind the pixel pass -- keys, the
// stable sort by Gaussian id, the per-Gaussian sum in double and chain (aux_math.h aux_bwd_chain).  Defined in aux_bwd.hip.
#pragma once
#include "common.h"

namespace r3 {

// what the per-Gaussian chain reads besides the state blobs, and the six outputs (any of them nullptr: not written)
struct AuxBwdGeom {
    const float *viewmatrix, *projmatrix;
    float tan_fovx, tan_fovy;
    const float *means3D, *scales;
    float scale_modifier;
    const float *rotations, *cov3D_precomp;
    const int* radii;
    float *dL_dmeans2D, *dL_dmeans3D, *dL_dopacity, *dL_dscales, *dL_drotations, *dL_dcov3D;
    bool any_output() const { return dL_dmeans2D || dL_dmeans3D || dL_dopacity || dL_dscales || dL_drotations || dL_dcov3D; }
};

// bytes of the workspace for a pair capacity R > 0 (asks rocPRIM once per R: call it outside a capture first)
size_t aux_bwd_workspace_bytes(size_t R);
// the slab inside a workspace: [R][4 quadrants][8 floats], every (slot < num_pairs, quadrant) row written by the pixel pass
float* aux_bwd_slab(char* workspace, size_t R);
// P rows of zeros in every output that is asked for
void aux_bwd_zero_outputs(int P, const AuxBwdGeom& g, hipStream_t s);
// the pointer checks of a call that walks (`what`: the entry point's name, for the message)
void aux_bwd_check_geom(const char* what, const AuxBwdGeom& g);
// keys, sort, per-Gaussian sum and chain over a slab the pixel pass has been launched on, on the same stream
void aux_bwd_second_stage(const PassStates& st, int P, int R, int width, int height, const AuxBwdGeom& g, char* workspace,
                          hipStream_t s);

}  // namespace r3
