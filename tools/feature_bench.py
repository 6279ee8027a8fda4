"""Times the feature maps (include/r3dgs_features.h, csrc/feature_maps.hip) against the workaround they replace -- ceil(C / 3)
renders with override_color = F[:, c:c+3] over a black background -- on the same build, in alternating blocks, and appends one
JSON line per channel count to profiles/feature_maps_bench.jsonl.

    python tools/feature_bench.py [--workload metric_500k_1600x1062] [--channels 3 16 64] [--blocks 6] [--per-block 10]

Per C:
  * `forward`: r3dgs_feature_maps alone, over the blobs of a finished forward;
  * `backward_features` / `backward_all`: r3dgs_feature_maps_backward with dL_dfeatures alone (frozen geometry) and with
    every output;
  * `step`: a training step through r3dgs_render.render(features=F, features_geom_grad=True) with a loss on the image and on
    the feature map -- forward, map, and the two backwards;
  * `workaround`: the same gradients through the image render plus ceil(C / 3) colour renders of F's slices;
  * `colour`: the step with the image loss alone, for scale;
  * the workspace bytes of the backward.
No speed bar is set; the row states step / workaround.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch   # noqa: E402

import synth_scene as ss   # noqa: E402
from aux_bench import _Model   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402


def bench(args, C, w, cam, g):
    from types import SimpleNamespace as NS

    import r3dgs_render
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
    Cpad = 3 * ((C + 2) // 3)
    wf = torch.zeros(Cpad, H, W, device="cuda")
    wf[:C] = dev(rng.uniform(-1, 1, (C, H, W)).astype(np.float32) / (H * W))
    F = dev(rng.uniform(0, 1, (P, C)).astype(np.float32)).requires_grad_(True)

    def clear():
        F.grad = None
        for t in pc.leaves():
            t.grad = None

    def colour():
        clear()
        (r3dgs_render.render(view, pc, pipe, bg)["render"] * wimg).sum().backward()

    def step():
        clear()
        out = r3dgs_render.render(view, pc, pipe, bg, features=F, features_geom_grad=True)
        ((out["render"] * wimg).sum() + (out["features"] * wf[:C]).sum()).backward()

    def workaround():
        clear()
        loss = (r3dgs_render.render(view, pc, pipe, bg)["render"] * wimg).sum()
        Fp = torch.nn.functional.pad(F, (0, Cpad - C))
        for c in range(0, Cpad, 3):
            loss = loss + (r3dgs_render.render(view, pc, pipe, black, override_color=Fp[:, c:c + 3])["render"] * wf[c:c + 3]).sum()
        loss.backward()

    none = torch.Tensor([])
    with torch.no_grad():
        scales, rotations = pc.get_scaling.contiguous(), pc.get_rotation.contiguous()
        fargs = (bg, pc._xyz.detach(), none, pc._opacity.detach(), scales, rotations, 1.0, none, view.world_view_transform,
                 view.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]), pc._degrees, view.camera_center, False, False)
        _C.hint_next_forward(True)
        fout = _C._forward_common(None, *fargs, exact=True)
    R, _, radii, geom, binning, img = fout
    Fd, gd = F.detach(), wf[:C].contiguous()

    def forward():
        _C.feature_maps(P, R, H, W, geom, binning, img, Fd)

    def backward(want):
        _C.feature_maps_backward(P, R, H, W, geom, binning, img, view.world_view_transform, view.full_proj_transform, cam.tanfovx,
                                 cam.tanfovy, pc._xyz.detach(), scales, 1.0, rotations, none, radii, Fd, gd, want=want)
    arms = dict(forward=forward, backward_features=lambda: backward(("features",)), backward_all=lambda: backward(_C.FEATURE_GRADS),
                step=step, workaround=workaround, colour=colour)
    for fn in arms.values():
        for _ in range(3):
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
    return dict(tool="feature_bench", workload=args.workload, C=C, P=P, W=W, H=H, pairs=int(R.pairs), blocks=args.blocks,
                per_block=args.per_block, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
                step_over_workaround=round(med["step"] / med["workaround"], 3),
                workspace_bytes=int(_C._lib.r3dgs_feature_maps_backward_workspace_bytes(P, int(R.capacity), C, W, H)),
                note="events around per_block back-to-back iterations of each arm (host gaps included); step / workaround / colour "
                     "are whole training steps: forward(s), loss arithmetic in torch, backward(s)",
                library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 16, 64])
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_maps_bench.jsonl"))
    args = ap.parse_args()
    w, cam, g = ss.make_workload(args.workload)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for C in args.channels:
        row = bench(args, C, w, cam, g)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
