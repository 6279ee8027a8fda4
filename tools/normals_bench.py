"""Times the surface-normal calls (include/r3dgs_normals.h, csrc/normals.hip, reduced-3dgs_amd/r3dgs_normals.py) against the same
operators written as torch lines, in alternating blocks, measures the accuracy of the depth normal against the float64
reference at the workload's size, and appends one JSON line to profiles/normals_bench.jsonl.

    python tools/normals_bench.py [--workload metric_500k_1600x1062] [--blocks 6] [--per-block 10]

Per block:
  * `gaussian_normals` / `gaussian_normals_torch`: the per-Gaussian view-space normals from the raw parameters, forward and
    backward (normalize, build_rotation, argmin, gather, dot, where, matmul in torch);
  * `consistency` / `consistency_torch`: depth -> normal -> loss on "depth" / "alpha" / "normal" maps, forward and backward
    (2DGS's depth_to_normal with slices and pads in torch);
  * `step` / `step_torch`: a training step -- render(aux, aux_grad, normals, features_geom_grad), image sum + 0.05 Ln, backward --
    with the unit's calls and with the torch lines (the torch normals ride render(features=...)), and `step_plain`: render and the
    image sum alone.
Events around per_block back-to-back calls; medians over the blocks, every block's figure beside them.  Back-to-back calls on
the same tensors are cache-warm.  No speed bar is set.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch   # noqa: E402

import r3dgs_normals as rn   # noqa: E402
import r3dgs_render   # noqa: E402
import synth_scene as ss   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402


class Pipe:
    debug = compute_cov3D_python = convert_SHs_python = False


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the same operators as torch lines (autograd; the dtype of their inputs) -----------------------------------------------------

def gaussian_normals_torch(xyz, scaling, rotation, rs):
    q = torch.nn.functional.normalize(rotation)
    r, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                     1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                     1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    k = torch.argmin(scaling, dim=1)
    n = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1)).squeeze(-1)
    facing = (n.detach() * (xyz.detach() - rs.campos)).sum(-1, keepdim=True)
    n = torch.where(facing > 0, -n, n)
    return n @ rs.viewmatrix[:3, :3]


def depth_to_normal_torch(depth, alpha, rs):
    H, W = depth.shape[-2:]
    live = alpha >= rn.ALPHA_MIN
    z = torch.where(live, depth / torch.where(live, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))[0]
    xs = (2 * (torch.arange(W, device=z.device, dtype=z.dtype) + 0.5) / W - 1) * rs.tanfovx
    ys = (2 * (torch.arange(H, device=z.device, dtype=z.dtype) + 0.5) / H - 1) * rs.tanfovy
    points = torch.stack([xs[None, :] * z, ys[:, None] * z, z], -1)
    dx = points[2:, 1:-1] - points[:-2, 1:-1]
    dy = points[1:-1, 2:] - points[1:-1, :-2]
    n = torch.nn.functional.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
    return torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1))


def consistency_torch(normal, depth, alpha, rs):
    n = depth_to_normal_torch(depth, alpha, rs)
    return (1 - alpha.detach()[0] * (normal * n).sum(0)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.jsonl"))
    args = ap.parse_args()
    w, cam, g = ss.make_workload(args.workload)
    P, W, H = w["P"], w["W"], w["H"]
    camera = types.SimpleNamespace(FoVx=cam.FoVx, FoVy=cam.FoVy, image_height=H, image_width=W,
                                   world_view_transform=dv(cam.world_view_transform), full_proj_transform=dv(cam.full_proj_transform),
                                   camera_center=dv(cam.camera_center))
    pc = types.SimpleNamespace(active_sh_degree=3, max_sh_degree=3, _degrees=dv(g["degrees"]))
    for name, a in (("_xyz", g["means3D"]), ("_features_dc", g["sh"][:, :1]), ("_features_rest", g["sh"][:, 1:]),
                    ("_opacity", g["opacity"]), ("_scaling", np.log(g["scales"])), ("_rotation", g["rotations"])):
        setattr(pc, name, torch.nn.Parameter(dv(a.astype(np.float32))))
    params = [pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation]
    bg = dv(np.zeros(3, np.float32))
    rs = r3dgs_render._settings(camera, pc, Pipe, bg, 1.0)
    with torch.no_grad():
        maps = r3dgs_render.render(camera, pc, Pipe, bg, aux=("depth", "alpha"), normals=True)
    depth, alpha, normal = (maps[k].detach().clone().requires_grad_() for k in ("depth", "alpha", "normal"))
    g3 = torch.randn(P, 3, device="cuda")

    def zero_grads():
        for p in params + [depth, alpha, normal]:
            p.grad = None

    def normals_arm(fn):
        zero_grads()
        fn().backward(g3)

    def consistency_arm(fn):
        zero_grads()
        fn().backward()

    def step(mode):
        zero_grads()
        if mode == "plain":
            out = r3dgs_render.render(camera, pc, Pipe, bg)
            loss = out["render"].sum()
        elif mode == "hip":
            out = r3dgs_render.render(camera, pc, Pipe, bg, aux=("depth", "alpha"), aux_grad=True, normals=True, features_geom_grad=True)
            loss = out["render"].sum() + 0.05 * rn.normal_consistency(out["normal"], out["depth"], rs, alpha=out["alpha"])[0]
        else:
            n = gaussian_normals_torch(pc._xyz, pc._scaling, pc._rotation, rs)
            out = r3dgs_render.render(camera, pc, Pipe, bg, aux=("depth", "alpha"), aux_grad=True, features=n, features_geom_grad=True)
            loss = out["render"].sum() + 0.05 * consistency_torch(out["features"], out["depth"], out["alpha"], rs)
        loss.backward()
        return loss

    arms = {
        "gaussian_normals": lambda: normals_arm(lambda: rn.gaussian_normals(pc._xyz, pc._scaling, pc._rotation, rs, raw=True)),
        "gaussian_normals_torch": lambda: normals_arm(lambda: gaussian_normals_torch(pc._xyz, pc._scaling, pc._rotation, rs)),
        "consistency": lambda: consistency_arm(lambda: rn.normal_consistency(normal, depth, rs, alpha=alpha)[0]),
        "consistency_torch": lambda: consistency_arm(lambda: consistency_torch(normal, depth, alpha, rs)),
        "step": lambda: step("hip"),
        "step_torch": lambda: step("torch"),
        "step_plain": lambda: step("plain"),
    }
    # accuracy of the depth normal at this size: the unit's, and the torch lines' in fp32, against the torch lines in float64
    with torch.no_grad():
        ref64 = depth_to_normal_torch(depth.double(), alpha.double(), rs)
        live = ref64.abs().sum(0) > 0
        ours = rn.depth_to_normal(depth.detach(), rs, alpha=alpha.detach())
        lines = depth_to_normal_torch(depth.detach(), alpha.detach(), rs)
        agree = {
            "depth_normal_abs_err": float((ours.double() - ref64).abs().max()),
            "depth_normal_abs_err_torch_fp32": float(((lines.double() - ref64) * live).abs().max()),
            "gaussian_normals_abs_err": float((rn.gaussian_normals(pc._xyz, pc._scaling, pc._rotation, rs, raw=True).double() -
                                               gaussian_normals_torch(pc._xyz.double(), pc._scaling.double(), pc._rotation.double(),
                                                                      types.SimpleNamespace(campos=rs.campos.double(),
                                                                                            viewmatrix=rs.viewmatrix.double()))).abs().max()),
        }
    for fn in arms.values():   # warm-up
        fn()
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in arms}
    for _ in range(args.blocks):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.per_block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.per_block)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = dict(tool="normals_bench", workload=args.workload, P=P, W=W, H=H, blocks=args.blocks, per_block=args.per_block,
               **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               **agree,
               note="events around per_block back-to-back calls, forward and backward; back-to-back calls on the same tensors are "
                    "cache-warm; the accuracy figures are maxima over the image against the torch lines in float64",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
