"""Times the absolute-gradient backward (r3dgs_backward_absgrad; csrc/blend.hip ABS instantiations, csrc/absgrad.hip) against
the plain one on the same build, in alternating blocks, and appends one JSON line per run to profiles/absgrad_bench.jsonl.

    python tools/absgrad_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 20]

  * `step`: a training step through r3dgs_render.render -- forward, image loss, backward -- with absgrad=True against False,
    between two events around a block of back-to-back steps (the figure includes the gaps between launches and, with the option
    on, the two tensors the backward allocates for the abs output and the workspace);
  * `stage`: the library's own stage timer on `blend_bwd` (HIP events around unit order + blend kernel + the abs reduction +
    pair reduction) and on `blend_bwd_kernel` (the blend kernel alone), abs against plain.
Medians over the blocks, and their range.  No bar is set; the estimate from the code was a backward blend about 15 % slower
with the option on.  Needs an MI355X."""
import argparse
import json
import math
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


class _Model:
    """The reference's GaussianModel, as far as r3dgs_render.render looks at it."""

    def __init__(self, g, dev):
        sh = dev(g["sh"])
        self._xyz = dev(g["means3D"]).requires_grad_(True)
        self._features_dc = sh[:, :1].contiguous().requires_grad_(True)
        self._features_rest = sh[:, 1:].contiguous().requires_grad_(True)
        self._opacity = dev(g["opacity"]).requires_grad_(True)
        self._scaling = dev(np.log(g["scales"]).astype(np.float32)).requires_grad_(True)
        self._rotation = dev(g["rotations"]).requires_grad_(True)
        self._degrees, self.active_sh_degree, self.max_sh_degree = dev(g["degrees"]), 3, 3

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))


class _Pipe:
    debug = compute_cov3D_python = convert_SHs_python = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absgrad_bench.jsonl"))
    args = ap.parse_args()
    import r3dgs_render

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w, cam, g = ss.make_workload(args.workload)
    W, H = w["W"], w["H"]
    view = type("Cam", (), {})()
    view.FoVx, view.FoVy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    view.image_height, view.image_width = H, W
    view.world_view_transform, view.full_proj_transform = dev(cam.world_view_transform), dev(cam.full_proj_transform)
    view.camera_center = dev(cam.camera_center)
    pc, bg = _Model(g, dev), dev(np.array([0.1, 0.2, 0.3], np.float32))
    dl = dev(ss.upstream_grad(W, H, seed=1))

    def step(absgrad):
        out = r3dgs_render.render(view, pc, _Pipe, bg, absgrad=absgrad)
        (out["render"] * dl).sum().backward()

    def block(absgrad, stages):
        if stages:
            _C.profile_enable(True, only=("blend_bwd", "blend_bwd_kernel"))
            _C.profile_read()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.per_block):
            step(absgrad)
        t1.record()
        torch.cuda.synchronize()
        if not stages:
            return t0.elapsed_time(t1) / args.per_block
        got = _C.profile_read()
        _C.profile_enable(False)
        return {k: got[k][0] / max(got[k][1], 1) for k in ("blend_bwd", "blend_bwd_kernel")}
    for _ in range(30):   # clocks, graphs and the reservation settle
        step(True)
        step(False)
    res = {"step": {True: [], False: []}, "blend_bwd": {True: [], False: []}, "blend_bwd_kernel": {True: [], False: []}}
    for _ in range(args.blocks):
        for on in (False, True):
            res["step"][on].append(block(on, False))
        for on in (False, True):
            st = block(on, True)
            for k, v in st.items():
                res[k][on].append(v)

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    row = {"tool": "absgrad_bench", "time": time.strftime("%Y-%m-%d %H:%M:%S"), "workload": args.workload, "blocks": args.blocks,
           "per_block": args.per_block, "library": _C.version()}
    for k, v in res.items():
        row[k] = {"plain": summary(v[False]), "absgrad": summary(v[True]),
                  "ratio": round(statistics.median(v[True]) / statistics.median(v[False]), 4)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
