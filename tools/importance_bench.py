"""Times the blend-contribution scores (include/r3dgs_importance.h, csrc/importance.hip) on one build, in alternating blocks,
and appends one JSON line per run to profiles/importance_bench.jsonl.

    python tools/importance_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 20]

Per block, over the blobs of one finished forward (as tools/aux_bench.py alternates its arms):
  * `call`: r3dgs_contribution_scores alone -- all four outputs, no weight map -- between two events;
  * `workaround`: the only way to the sum before this call existed, on the same state -- r3dgs_feature_maps_backward with
    C = 1, F = 1 and an all-ones upstream gradient, features only -- between two events;
  * `blend_fwd`: the forward blend stage of the same scene, by the library's own stage timer, for scale.
Medians over the blocks, with every block's figure beside them.  No speed bar is set.  Needs an MI355X."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "importance_bench.jsonl"))
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
    ones_f, ones_g = torch.ones(P, 1, device="cuda"), torch.ones(1, H, W, device="cuda")
    out = {k: torch.empty(P, dtype=_C._SCORE_DTYPES[k], device="cuda") for k in _C.SCORES}

    def call(fout):
        R, _, _, geom, binning, img = fout
        _C.contribution_scores(P, R, H, W, geom, binning, img, out=out)

    def workaround(fout):
        R, _, radii, geom, binning, img = fout
        return _C.feature_maps_backward(P, R, H, W, geom, binning, img, None, None, 1.0, 1.0, None, None, 1.0, None, None, radii,
                                        ones_f, ones_g, want=("features",))
    for _ in range(5):
        call(fout)
        got = workaround(fout)
    torch.cuda.synchronize()
    agree = float(((out["sum"] - got["features"][:, 0].double()).abs() / out["count"].clamp(min=1)).max())
    arms = dict(call=call, workaround=workaround)
    ms = {k: [] for k in ("blend_fwd", *arms)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        _C.profile_enable(True, only=["blend_fwd"])
        _C.profile_read()
        for _ in range(args.per_block):
            fout = forward()
        torch.cuda.synchronize()
        total, launches = _C.profile_read()["blend_fwd"]
        _C.profile_enable(False)
        ms["blend_fwd"].append(total / max(launches, 1))
        for name, fn in arms.items():
            e0.record()
            for _ in range(args.per_block):
                fn(fout)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.per_block)
    med = {k: statistics.median(v) for k, v in ms.items()}
    R = fout[0]
    row = dict(tool="importance_bench", workload=args.workload, P=P, W=W, H=H, pairs=int(R.pairs), blocks=args.blocks,
               per_block=args.per_block, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               call_over_workaround=round(med["call"] / med["workaround"], 3), call_over_blend_fwd=round(med["call"] / med["blend_fwd"], 3),
               workspace_bytes=int(_C._lib.r3dgs_contribution_scores_workspace_bytes(P, int(R.capacity), W, H)),
               workaround_workspace_bytes=int(_C._lib.r3dgs_feature_maps_backward_workspace_bytes(P, int(R.capacity), 1, W, H)),
               sum_against_workaround_per_count=agree, gaussians_seen=int((out["count"] > 0).sum()),
               note="call / workaround: events around per_block back-to-back calls (launch gaps and the per-call workspace allocation "
                    "included); blend_fwd: the library's stage timer",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
