"""Times the auxiliary-map pass (include/r3dgs_aux.h, csrc/aux_maps.hip) against the forward blend stage of the same scene,
on the same build, in alternating blocks, and appends one JSON line per run to profiles/aux_maps_bench.jsonl.

    python tools/aux_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 20]

A block of forwards with the library's own stage timer on `blend_fwd` (HIP events around the forward blend kernel), then a
block of aux launches over the blobs of the last forward between two events; medians over the blocks.  The aux pass walks
what the forward blend walks, without the colour: the expectation from the code is a time at or below that stage's.  Needs
an MI355X.

    python tools/aux_bench.py --backward [--blocks 6] [--per-block 10]

times the gradients through the maps (r3dgs_aux_maps_backward, csrc/aux_bwd.hip) instead and appends to
profiles/aux_grad_bench.jsonl, again in alternating blocks on one build:
  * `call`: the new call alone, over the blobs of a finished forward, upstream gradients for depth and alpha;
  * `step`: a training step through r3dgs_render.render(aux=("depth", "alpha"), aux_grad=True) with a loss on the image, the
    depth and the alpha map -- forward, maps, and the two backwards;
  * `workaround`: the same gradients without the feature -- a second render with override_color = (z, 1, 0) over a black
    background (z the view depth, built in torch so that its gradient reaches xyz): two forwards, two colour backwards;
  * `colour`: the step with the image loss alone, for scale.
No speed bar is set; the row states step / workaround."""
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

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def backward_bench(args):
    from types import SimpleNamespace as NS

    import r3dgs_render
    w, cam, g = ss.make_workload(args.workload)
    P, H, W = w["P"], w["H"], w["W"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pc = _Model(g, dev)
    view = NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg, black = dev(np.array([0.1, 0.3, 0.2], np.float32)), dev(np.zeros(3, np.float32))
    rng = np.random.default_rng(1)
    wimg = dev(rng.uniform(-1, 1, (3, H, W)).astype(np.float32) / (H * W))
    wd, wa = (dev(rng.uniform(-1, 1, (1, H, W)).astype(np.float32) / (H * W)) for _ in range(2))

    def clear():
        for t in pc.leaves():
            t.grad = None

    def colour():
        clear()
        (r3dgs_render.render(view, pc, pipe, bg)["render"] * wimg).sum().backward()

    def step():
        clear()
        out = r3dgs_render.render(view, pc, pipe, bg, aux=("depth", "alpha"), aux_grad=True)
        ((out["render"] * wimg).sum() + (out["depth"] * wd).sum() + (out["alpha"] * wa).sum()).backward()

    def workaround():
        clear()
        out = r3dgs_render.render(view, pc, pipe, bg)
        z = pc._xyz @ view.world_view_transform[:3, 2] + view.world_view_transform[3, 2]
        second = r3dgs_render.render(view, pc, pipe, black, override_color=torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1))
        ((out["render"] * wimg).sum() + (second["render"][0:1] * wd).sum() + (second["render"][1:2] * wa).sum()).backward()

    # the call alone: over the blobs of one forward of the activated model
    none = torch.Tensor([])
    with torch.no_grad():
        scales, rotations = pc.get_scaling.contiguous(), pc.get_rotation.contiguous()
        fargs = (bg, pc._xyz.detach(), none, pc._opacity.detach(), scales, rotations, 1.0, none, view.world_view_transform,
                 view.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]), pc._degrees, view.camera_center, False, False)
        _C.hint_next_forward(True)
        fout = _C._forward_common(None, *fargs, exact=True)
    R, _, radii, geom, binning, img = fout
    gD, gA = wd.reshape(-1).contiguous(), wa.reshape(-1).contiguous()

    def call():
        _C.aux_maps_backward(P, R, H, W, geom, binning, img, view.world_view_transform, view.full_proj_transform, cam.tanfovx,
                             cam.tanfovy, pc._xyz.detach(), scales, 1.0, rotations, none, radii, gD, gA, None)
    arms = dict(call=call, step=step, workaround=workaround, colour=colour)
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
    row = dict(tool="aux_bench --backward", workload=args.workload, P=P, W=W, H=H, pairs=int(R.pairs), blocks=args.blocks,
               per_block=args.per_block, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               step_over_workaround=round(med["step"] / med["workaround"], 3),
               workspace_bytes=int(_C._lib.r3dgs_aux_maps_backward_workspace_bytes(P, int(R.capacity), W, H)),
               note="events around per_block back-to-back iterations of each arm (host gaps included); step / workaround / colour "
                    "are whole training steps: forward(s), loss arithmetic in torch, backward(s)",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    out = args.out or os.path.join(ROOT, "profiles", "aux_grad_bench.jsonl")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="time the gradients through the maps (see the module's docstring)")
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=None, help="default: profiles/aux_maps_bench.jsonl, or profiles/aux_grad_bench.jsonl with --backward")
    args = ap.parse_args()
    if args.backward:
        return backward_bench(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "aux_maps_bench.jsonl")
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
