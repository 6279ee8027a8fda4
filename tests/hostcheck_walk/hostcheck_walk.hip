// Host shim of the replay passes' index arithmetic (reduced-3dgs_amd/csrc/replay_walk.h): the R3_HD functions a lane
// executes -- xcd_remap, quad_lane, walk_span -- called on the CPU, and of the host plan of a replay backward
// (pass_driver.h replay_bwd_plan).  Loaded with ctypes by tests/test_replay_walk_cpu.py; as a program (its main below, built
// plainly and under the host sanitizers by the same test) it checks the plan's whole truth table itself.
#include <cstdio>

#include "../../reduced-3dgs_amd/csrc/pass_driver.h"
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

// 0 = Nothing, 1 = ZeroOutputs, 2 = Walk
int hw_replay_bwd_plan(int P, int R, int has_upstream, int any_output)
{
    return (int)replay_bwd_plan(P, R, has_upstream != 0, any_output != 0);
}

}  // extern "C"

// The plan over P, R in {0, 1} x upstream yes / no x outputs yes / no, against the order the contract states: P == 0 first,
// then "nothing to walk", then "nothing asked for".  Prints one row per case; exit status 1 on a mismatch.
int main()
{
    // by c = P | R << 1 | upstream << 2 | outputs << 3, written out: no expression shared with replay_bwd_plan
    static const int kPlanTable[16] = {0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 2};
    int bad = 0;
    for (int c = 0; c < 16; c++) {
        const int P = c & 1, R = (c >> 1) & 1, up = (c >> 2) & 1, outs = (c >> 3) & 1;
        const int want = kPlanTable[c];
        const int got = hw_replay_bwd_plan(P, R, up, outs);
        std::printf("P=%d R=%d upstream=%d outputs=%d plan=%d\n", P, R, up, outs, got);
        bad += got != want;
    }
    return bad ? 1 : 0;
}
