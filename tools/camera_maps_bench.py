"""Times the maps' share of a camera gradient (include/r3dgs_camera.h r3dgs_camera_backward_maps, render(camera_grad_maps=True))
at the metric shape and appends one JSON line per run to profiles/camera_maps_bench.jsonl.

    python tools/camera_maps_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 10] [--out FILE]

Four arms on one build, in alternating blocks (a block of each arm in turn, repeated; medians over the blocks), as
tools/aux_bench.py does:
  * `call_maps`: r3dgs_camera_backward_maps alone, over the screen-space sums of a finished aux_maps_backward_screen;
  * `call_colour`: r3dgs_camera_backward alone (the colour route's pass), over the sums of a finished backward;
  * `track_maps`: a tracking step with a FROZEN model and a colour + depth + alpha loss through ONE render with aux_grad=True,
    camera_grad_maps=True: forward, maps, loss arithmetic in torch, the colour backward with its camera pass, the maps'
    _screen backward with its camera pass;
  * `track_two_renders`: the same loss by the workaround -- the colour render, and a second render with override_color =
    stack(z(V), 1, 0) over black whose first two channels are the depth and alpha maps -- both through the colour route's
    camera gradients.
The ratio track_maps / track_two_renders is recorded whichever way it falls; no speed bar is set.  Needs an MI355X."""
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
    """The reference's GaussianModel, as far as r3dgs_render.render looks at it; frozen: nothing requires grad."""

    def __init__(self, g, dev):
        sh = dev(g["sh"])
        self._xyz = dev(g["means3D"])
        self._features_dc, self._features_rest = sh[:, :1].contiguous(), sh[:, 1:].contiguous()
        self._opacity = dev(g["opacity"])
        self._scaling = dev(np.log(g["scales"]).astype(np.float32))
        self._rotation = dev(g["rotations"])
        self._degrees, self.active_sh_degree, self.max_sh_degree = dev(g["degrees"]), 3, 3

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_maps_bench.jsonl"))
    args = ap.parse_args()
    import r3dgs_render
    w, cam, g = ss.make_workload(args.workload)
    P, H, W = w["P"], w["H"], w["W"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pc = _Model(g, dev)
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg, black = dev(np.array([0.1, 0.3, 0.2], np.float32)), torch.zeros(3, device="cuda")
    rng = np.random.default_rng(1)
    wimg = dev(rng.uniform(-1, 1, (3, H, W)).astype(np.float32) / (H * W))
    wdepth, walpha = (dev(rng.uniform(-1, 1, (1, H, W)).astype(np.float32) / (H * W)) for _ in range(2))
    ones = torch.ones(P, 1, device="cuda")

    def view():
        return NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy,
                  world_view_transform=dev(cam.world_view_transform).requires_grad_(True),
                  full_proj_transform=dev(cam.full_proj_transform).requires_grad_(True),
                  camera_center=dev(cam.camera_center).requires_grad_(True))
    v = view()

    def clear():
        for t in (v.world_view_transform, v.full_proj_transform, v.camera_center):
            t.grad = None

    def track_maps():
        clear()
        out = r3dgs_render.render(v, pc, pipe, bg, aux=("depth", "alpha"), aux_grad=True, camera_grad_maps=True)
        ((out["render"] * wimg).sum() + (out["depth"] * wdepth).sum() + (out["alpha"] * walpha).sum()).backward()

    def track_two_renders():
        clear()
        out = r3dgs_render.render(v, pc, pipe, bg)
        z = (torch.cat([pc._xyz, ones], 1) @ v.world_view_transform)[:, 2:3]
        second = r3dgs_render.render(v, pc, pipe, black, override_color=torch.cat([z, ones, torch.zeros_like(ones)], 1))["render"]
        ((out["render"] * wimg).sum() + (second[0:1] * wdepth).sum() + (second[1:2] * walpha).sum()).backward()

    # the two calls alone: over one exact forward, the colour backward's sums and the aux maps' screen-space sums
    vm, pm, cp = (t.detach() for t in (v.world_view_transform, v.full_proj_transform, v.camera_center))
    xyz, dc, rest, opacity, scaling, rotation = (pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation)
    with torch.no_grad():
        _C.hint_next_forward(True)
        R, _, radii, geom, binning, img = _C.rasterize_gaussian_params(bg, xyz, dc, rest, pc._degrees, opacity, scaling, rotation, 1.0,
                                                                       vm, pm, cam.tanfovx, cam.tanfovy, H, W, cp, False, False,
                                                                       exact=True)
        back = _C.rasterize_gaussian_params_backward(bg, xyz, radii, dc, rest, pc._degrees, opacity, scaling, rotation, 1.0, vm, pm,
                                                     cam.tanfovx, cam.tanfovy, wimg, cp, geom, R, binning, img, 0.0, False,
                                                     _want_2d=True)
        sc, rot = pc.get_scaling.contiguous(), pc.get_rotation.contiguous()
        scr = _C.aux_maps_backward_screen(P, R, H, W, geom, binning, img, vm, pm, cam.tanfovx, cam.tanfovy, xyz, sc, 1.0, rot, None,
                                          radii, wdepth, walpha, None, want=("means2D",) + _C.SCREEN_GRADS)
    g2, gcol, gcon = back[0], back[7], back[8]

    def call_colour():
        _C.camera_backward(xyz, pc._degrees, dc, rest, scaling, rotation, 1.0, None, True, vm, pm, cp, cam.tanfovx, cam.tanfovy, H, W,
                           radii, geom, g2, gcon, gcol)

    def call_maps():
        _C.camera_backward_maps(xyz, sc, rot, 1.0, None, vm, pm, cam.tanfovx, cam.tanfovy, H, W, radii, scr["means2D"], scr["conic"],
                                scr["z"])
    arms = dict(call_maps=call_maps, call_colour=call_colour, track_maps=track_maps, track_two_renders=track_two_renders)
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
    med = {k: statistics.median(x) for k, x in ms.items()}
    row = dict(tool="camera_maps_bench", workload=args.workload, P=P, W=W, H=H, visible=int((radii > 0).sum()), blocks=args.blocks,
               per_block=args.per_block, **{f"{k}_ms": round(x, 4) for k, x in med.items()},
               **{f"{k}_ms_blocks": [round(y, 4) for y in x] for k, x in ms.items()},
               call_maps_over_call_colour=round(med["call_maps"] / med["call_colour"], 3),
               track_maps_over_track_two_renders=round(med["track_maps"] / med["track_two_renders"], 3),
               note="events around per_block back-to-back iterations of each arm (host gaps included: the calls are two launches "
                    "and their wrappers' checks); the tracking steps are whole steps with a frozen model: forward(s), loss "
                    "arithmetic in torch, backward(s), every camera pass; the two-render arm cannot carry a median-depth loss",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
