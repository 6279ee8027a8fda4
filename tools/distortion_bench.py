"""Times the depth-distortion passes (include/r3dgs_distortion.h, csrc/distortion.hip) against the auxiliary-map passes of the
same state (include/r3dgs_aux.h), on one build, in alternating blocks, and appends one JSON line per run to
profiles/distortion_bench.jsonl.

    python tools/distortion_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 10] [--near 0.2 --far 100]

Arms, each timed by HIP events around `per_block` back-to-back iterations (host gaps included), medians over the blocks:
  * `dist_fwd` : _C.distortion_map with the saved moments          against  `aux_fwd`: _C.aux_maps, all three maps
  * `dist_bwd` : _C.distortion_map_backward                         against  `aux_bwd`: _C.aux_maps_backward (depth and alpha)
    -- all four over the blobs of one finished forward of the activated model;
  * `step_dist`: a training step through r3dgs_render.render(distortion=(near, far)) with a loss on the image and the map
    against  `step_colour`: the step with the image loss alone.
No ratio is required; the row states the three ratios.  Needs an MI355X."""
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

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--near", type=float, default=0.2)
    ap.add_argument("--far", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.jsonl"))
    args = ap.parse_args()
    import r3dgs_render
    w, cam, g = ss.make_workload(args.workload)
    P, H, W = w["P"], w["H"], w["W"]
    mapping = _C.depth_mapping((args.near, args.far))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pc = _Model(g, dev)
    view = NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = dev(np.array([0.1, 0.3, 0.2], np.float32))
    rng = np.random.default_rng(1)
    wimg = dev(rng.uniform(-1, 1, (3, H, W)).astype(np.float32) / (H * W))
    wd, wa = (dev(rng.uniform(-1, 1, (1, H, W)).astype(np.float32) / (H * W)) for _ in range(2))

    def clear():
        for t in pc.leaves():
            t.grad = None

    def step_colour():
        clear()
        (r3dgs_render.render(view, pc, pipe, bg)["render"] * wimg).sum().backward()

    def step_dist():
        clear()
        out = r3dgs_render.render(view, pc, pipe, bg, distortion=mapping)
        ((out["render"] * wimg).sum() + (out["distortion"] * wd).sum()).backward()

    none = torch.Tensor([])
    with torch.no_grad():
        scales, rotations = pc.get_scaling.contiguous(), pc.get_rotation.contiguous()
        fargs = (bg, pc._xyz.detach(), none, pc._opacity.detach(), scales, rotations, 1.0, none, view.world_view_transform,
                 view.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]), pc._degrees, view.camera_center, False, False)
        _C.hint_next_forward(True)
        fout = _C._forward_common(None, *fargs, exact=True)
    R, _, radii, geom, binning, img = fout
    gD, gA = wd.reshape(-1).contiguous(), wa.reshape(-1).contiguous()
    _, moments = _C.distortion_map(P, R, H, W, geom, binning, img, *mapping, want_moments=True)
    model = (view.world_view_transform, view.full_proj_transform, cam.tanfovx, cam.tanfovy, pc._xyz.detach(), scales, 1.0, rotations,
             none, radii)

    def dist_fwd():
        _C.distortion_map(P, R, H, W, geom, binning, img, *mapping, want_moments=True)

    def aux_fwd():
        _C.aux_maps(P, R, H, W, geom, binning, img)

    def dist_bwd():
        _C.distortion_map_backward(P, R, H, W, geom, binning, img, *model, gD, moments, *mapping)

    def aux_bwd():
        _C.aux_maps_backward(P, R, H, W, geom, binning, img, *model, gD, gA, None)
    arms = dict(dist_fwd=dist_fwd, aux_fwd=aux_fwd, dist_bwd=dist_bwd, aux_bwd=aux_bwd, step_dist=step_dist, step_colour=step_colour)
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
    row = dict(tool="distortion_bench", workload=args.workload, P=P, W=W, H=H, pairs=int(R.pairs), near=mapping[0], far=mapping[1],
               blocks=args.blocks, per_block=args.per_block, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               dist_fwd_over_aux_fwd=round(med["dist_fwd"] / med["aux_fwd"], 3),
               dist_bwd_over_aux_bwd=round(med["dist_bwd"] / med["aux_bwd"], 3),
               step_dist_over_step_colour=round(med["step_dist"] / med["step_colour"], 3),
               workspace_bytes=int(_C._lib.r3dgs_distortion_map_backward_workspace_bytes(P, int(R.capacity), W, H)),
               note="events around per_block back-to-back iterations of each arm (host gaps included); the two steps are whole "
                    "training steps: forward, loss arithmetic in torch, backward(s)",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
