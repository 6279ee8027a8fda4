"""Times the camera gradients (include/r3dgs_camera.h, csrc/camera_bwd.hip) at the metric shape and appends one JSON line per
run to profiles/camera_grad_bench.jsonl.

    python tools/camera_grad_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 10]

Three arms on one build, in alternating blocks (block of arm A, block of arm B, ..., repeated; medians over the blocks):
  * `call`: r3dgs_camera_backward alone, over the state of a finished forward and the sums of a finished backward;
  * `step_camera`: a training step through r3dgs_render.render with a camera whose three tensors require grad -- forward, image
    loss in torch, backward, the camera pass;
  * `step`: the same step with a camera that asks for nothing, i.e. today's step.
From the code the operator moves about 120 B per visible Gaussian and 4 B per culled one; the row states the bytes that
expectation amounts to and the rate the measured time implies.  That is an expectation, not a pass criterion: no speed bar is
set.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace as NS

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

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_grad_bench.jsonl"))
    args = ap.parse_args()
    import r3dgs_render
    w, cam, g = ss.make_workload(args.workload)
    P, H, W = w["P"], w["H"], w["W"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pc = _Model(g, dev)
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = dev(np.array([0.1, 0.3, 0.2], np.float32))
    wimg = dev(np.random.default_rng(1).uniform(-1, 1, (3, H, W)).astype(np.float32) / (H * W))

    def view(grad):
        return NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy,
                  world_view_transform=dev(cam.world_view_transform).requires_grad_(grad),
                  full_proj_transform=dev(cam.full_proj_transform).requires_grad_(grad),
                  camera_center=dev(cam.camera_center).requires_grad_(grad))
    plain, refined = view(False), view(True)

    def step_of(v):
        def step():
            for t in pc.leaves() + (v.world_view_transform, v.full_proj_transform, v.camera_center):
                t.grad = None
            (r3dgs_render.render(v, pc, pipe, bg)["render"] * wimg).sum().backward()
        return step

    # the call alone: over one forward + backward of the raw-parameter route
    vm, pm, cp = plain.world_view_transform, plain.full_proj_transform, plain.camera_center
    raw = tuple(t.detach() for t in pc.leaves())
    xyz, dc, rest, opacity, scaling, rotation = raw
    with torch.no_grad():
        _C.hint_next_forward(True)
        R, _, radii, geom, binning, img = _C.rasterize_gaussian_params(bg, xyz, dc, rest, pc._degrees, opacity, scaling, rotation, 1.0,
                                                                       vm, pm, cam.tanfovx, cam.tanfovy, H, W, cp, False, False,
                                                                       exact=True)
        back = _C.rasterize_gaussian_params_backward(bg, xyz, radii, dc, rest, pc._degrees, opacity, scaling, rotation, 1.0, vm, pm,
                                                     cam.tanfovx, cam.tanfovy, wimg, cp, geom, R, binning, img, 0.0, False,
                                                     _want_2d=True)
    g2, gcol, gcon = back[0], back[7], back[8]

    def call():
        _C.camera_backward(xyz, pc._degrees, dc, rest, scaling, rotation, 1.0, None, True, vm, pm, cp, cam.tanfovx, cam.tanfovy, H, W,
                           radii, geom, g2, gcon, gcol)
    arms = dict(call=call, step_camera=step_of(refined), step=step_of(plain))
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.blocks):
        for name, fn in arms.items():
            e0.record()
            for _ in range(args.per_block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.per_block)
    med = {k: statistics.median(v) for k, v in ms.items()}
    visible = int((radii > 0).sum())
    expected = 120 * visible + 4 * (P - visible)
    row = dict(tool="camera_grad_bench", workload=args.workload, P=P, W=W, H=H, visible=visible, blocks=args.blocks,
               per_block=args.per_block, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               step_camera_over_step=round(med["step_camera"] / med["step"], 3), expected_bytes=expected,
               implied_GBps_of_expected_bytes=round(expected / (med["call"] * 1e-3) / 1e9, 1),
               workspace_bytes=int(_C._lib.r3dgs_camera_backward_workspace_bytes(P)),
               note="events around per_block back-to-back iterations of each arm (host gaps included: `call` is two launches and the "
                    "wrapper's checks, so its time is an upper bound on the kernels'); step / step_camera are whole training steps: "
                    "forward, loss arithmetic in torch, backward; expected_bytes is read off the code, not measured",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
