"""Times the auxiliary-map pass (include/r3dgs_aux.h, csrc/aux_maps.hip) against the forward blend stage of the same scene,
on the same build, in alternating blocks, and appends one JSON line per run to profiles/aux_maps_bench.jsonl.

    python tools/aux_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 20]

A block of forwards with the library's own stage timer on `blend_fwd` (HIP events around the forward blend kernel), then a
block of aux launches over the blobs of the last forward between two events; medians over the blocks.  The aux pass walks
what the forward blend walks, without the colour: the expectation from the code is a time at or below that stage's.  Needs
an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch   # noqa: E402

import synth_scene as ss   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_maps_bench.jsonl"))
    args = ap.parse_args()
    w, cam, g = ss.make_workload(args.workload)
    P, H, W = w["P"], w["H"], w["W"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    none = torch.Tensor([])
    fargs = (dev(np.zeros(3, np.float32)), dev(g["means3D"]), none, dev(g["opacity"]), dev(g["scales"]), dev(g["rotations"]), 1.0,
             none, dev(cam.world_view_transform), dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]),
             dev(g["degrees"]), dev(cam.camera_center), False, False)

    def forward():
        with torch.no_grad():
            return _C.rasterize_gaussians(*fargs)
    for _ in range(5):   # the first pass of a shape is the exact-size one; then the reserved path
        fout = forward()
    R, _, _, geom, binning, img = fout
    for _ in range(5):
        _C.aux_maps(P, R, H, W, geom, binning, img)
    torch.cuda.synchronize()
    blend_ms, aux_ms = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        _C.profile_enable(True, only=["blend_fwd"])
        _C.profile_read()
        for _ in range(args.per_block):
            fout = forward()
        torch.cuda.synchronize()
        ms, launches = _C.profile_read()["blend_fwd"]
        _C.profile_enable(False)
        blend_ms.append(ms / max(launches, 1))
        R, _, _, geom, binning, img = fout
        e0.record()
        for _ in range(args.per_block):
            _C.aux_maps(P, R, H, W, geom, binning, img)
        e1.record()
        torch.cuda.synchronize()
        aux_ms.append(e0.elapsed_time(e1) / args.per_block)
    row = dict(tool="aux_bench", workload=args.workload, P=P, W=W, H=H, pairs=int(R.pairs), blocks=args.blocks,
               per_block=args.per_block, blend_fwd_ms=round(statistics.median(blend_ms), 4),
               aux_maps_ms=round(statistics.median(aux_ms), 4), blend_fwd_ms_blocks=[round(x, 4) for x in blend_ms],
               aux_maps_ms_blocks=[round(x, 4) for x in aux_ms],
               aux_over_blend=round(statistics.median(aux_ms) / statistics.median(blend_ms), 3),
               note="aux: events around per_block back-to-back launches (launch gaps included); blend_fwd: the library's stage timer",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
