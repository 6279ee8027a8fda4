// Host shim of the replay passes' index arithmetic (reduced-3dgs_amd/csrc/replay_walk.h): the R3_HD functions a lane
// executes -- xcd_remap, quad_lane, walk_span -- called on the CPU.  Loaded with ctypes by tests/test_replay_walk_cpu.py.
#include "../../reduced-3dgs_amd/csrc/replay_walk.h"

using namespace r3;

extern "C" {

unsigned hw_xcd_remap(unsigned b, unsigned nblocks) { return xcd_remap(b, nblocks); }

// out = {tile, quad, px, py, inside, pix, qx0, qy0, pxf, pyf}
void hw_quad_lane(unsigned wg, int lane, int gx, int W, int H, long long* out)
{
    const QuadLane q = quad_lane(wg, lane, gx, W, H);
    out[0] = q.tile;
    out[1] = q.quad;
    out[2] = q.px;
    out[3] = q.py;
    out[4] = q.inside ? 1 : 0;
    out[5] = (long long)q.pix;
    out[6] = (long long)q.qx0;
    out[7] = (long long)q.qy0;
    out[8] = (long long)q.pxf;
    out[9] = (long long)q.pyf;
}

// out = {first, list_len, len}
void hw_walk_span(unsigned range_x, unsigned range_y, unsigned quad_depth, unsigned R, unsigned* out)
{
    const WalkSpan s = walk_span(make_uint2(range_x, range_y), quad_depth, R);
    out[0] = s.first;
    out[1] = s.list_len;
    out[2] = s.len;
}

int hw_tile() { return kTile; }

}  // extern "C"
