"""Times the anti-aliasing calls (include/r3dgs_mip.h, csrc/mip.hip, reduced-3dgs_amd/r3dgs_mip.py) against the same maps written
as torch lines and fed to the same rasterizer, in alternating blocks, and appends one JSON line to profiles/mip_bench.jsonl.

    python tools/mip_bench.py [--workload metric_500k_1600x1062] [--cameras 100] [--blocks 6] [--per-block 10]

Per block:
  * `compensation` / `compensation_torch`: the per-view 2D opacity compensation, forward and backward (gradients of means,
    opacity, scaling and rotation), from the raw parameters;
  * `filtered` / `filtered_torch`: the 3D filter applied to _scaling / _opacity, forward and backward;
  * `filter3d` / `filter3d_torch`: the 3D filter of a set of cameras (Mip-Splatting's compute_3D_filter loop in torch);
  * `step` / `step_torch`: a training step -- both maps, render() from the raw parameters, a sum loss, backward -- with the maps
    in HIP (render(antialiasing=True, filter_3d=f)) and as the torch lines (their outputs put into a view of the model), and
    `step_plain`: the same step with both filters off.
Events around per_block back-to-back calls; medians over the blocks, with every block's figure beside them.  The tensors of the
per-op arms fit the last-level cache: cache-warm figures.  No speed bar is set.  Needs an MI355X."""
import argparse
import json
import math
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

import r3dgs_mip as mip   # noqa: E402
import r3dgs_render   # noqa: E402
import synth_scene as ss   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402


class Pipe:
    debug = compute_cov3D_python = convert_SHs_python = False


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the same maps as torch lines (fp32, autograd) -------------------------------------------------------------------------

def rotation_matrix(q):
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                        1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                        1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def compensation_torch(xyz, opacity, scaling, rotation, rs):
    V = rs.viewmatrix
    fx, fy = rs.image_width / (2 * rs.tanfovx), rs.image_height / (2 * rs.tanfovy)
    M = rotation_matrix(torch.nn.functional.normalize(rotation)) * (rs.scale_modifier * torch.exp(scaling))[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    t = xyz @ V[:3, :3] + V[3, :3]
    z = t[:, 2]
    zs = torch.where(z > 0.2, z, torch.ones_like(z))
    tx = torch.clamp(t[:, 0] / zs, -1.3 * rs.tanfovx, 1.3 * rs.tanfovx) * zs
    ty = torch.clamp(t[:, 1] / zs, -1.3 * rs.tanfovy, 1.3 * rs.tanfovy) * zs
    zero = torch.zeros_like(zs)
    J = torch.stack([fx / zs, zero, -fx * tx / (zs * zs), zero, fy / zs, -fy * ty / (zs * zs)], -1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    C = A @ Sigma @ A.transpose(1, 2)
    a, b, c = C[:, 0, 0], C[:, 0, 1], C[:, 1, 1]
    rho = torch.sqrt(torch.clamp((a * c - b * b) / ((a + 0.3) * (c + 0.3) - b * b), min=0.000025))
    rho = torch.where(z > 0.2, rho, torch.ones_like(rho))
    p = torch.sigmoid(opacity) * rho[:, None]
    return torch.log(p) - torch.log1p(-p)


def filtered_torch(scaling, opacity, f):
    s2 = torch.square(torch.exp(scaling))
    s2f = s2 + torch.square(f)
    coef = torch.sqrt(s2.prod(dim=1) / s2f.prod(dim=1))
    p = torch.sigmoid(opacity) * coef[:, None]
    return torch.log(torch.sqrt(s2f)), torch.log(p) - torch.log1p(-p)


@torch.no_grad()
def filter3d_torch(xyz, table):
    P = xyz.shape[0]
    d = torch.full((P,), 100000.0, device=xyz.device)
    valid = torch.zeros(P, dtype=torch.bool, device=xyz.device)
    focal = 0.0
    for cam in table.cpu().tolist():   # the reference loops over Python camera objects: host scalars per camera
        V = torch.tensor(cam[:16], device=xyz.device).reshape(4, 4)
        fx, fy, W, H = cam[16:]
        t = xyz @ V[:3, :3] + V[3, :3]
        z = t[:, 2]
        zc = torch.clamp(z, min=0.001)
        x, y = t[:, 0] / zc * fx + W / 2.0, t[:, 1] / zc * fy + H / 2.0
        ok = (z > 0.2) & (x >= -0.15 * W) & (x <= W * 1.15) & (y >= -0.15 * H) & (y <= 1.15 * H)
        d[ok] = torch.min(d[ok], z[ok])
        valid |= ok
        focal = max(focal, fx)
    d[~valid] = d[valid].max()
    return (d / focal * (0.2 ** 0.5))[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062")
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip_bench.jsonl"))
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
    rows = []
    for v in range(args.cameras):   # the training set: the camera moved around a little
        c = ss.make_camera(W, H, w["f"], v)
        rows.append(np.concatenate([c.world_view_transform.reshape(16), [w["f"], w["f"], W, H]]))
    table = dv(np.asarray(rows, np.float32))
    f = mip.filter_3d(pc._xyz, table)
    f_torch = filter3d_torch(pc._xyz.detach(), table)
    g1, g3 = torch.randn(P, 1, device="cuda"), torch.randn(P, 3, device="cuda")

    def zero_grads():
        for p in params:
            p.grad = None

    def compensation(fn):
        zero_grads()
        fn().backward(g1)

    def filtered(fn):
        zero_grads()
        s, o = fn()
        torch.autograd.backward([s, o], [g3, g1])

    def step(mode):
        zero_grads()
        if mode == "hip":
            out = r3dgs_render.render(camera, pc, Pipe, bg, antialiasing=True, filter_3d=f)
        elif mode == "torch":
            s, o = filtered_torch(pc._scaling, pc._opacity, f)
            o = compensation_torch(pc._xyz, o, s, pc._rotation, rs)
            out = r3dgs_render.render(camera, r3dgs_render._FilteredModel(pc, s.contiguous(), o.contiguous()), Pipe, bg)
        else:
            out = r3dgs_render.render(camera, pc, Pipe, bg)
        out["render"].sum().backward()
        return out["render"]

    arms = {
        "compensation": lambda: compensation(lambda: mip.antialias_opacity(pc._xyz, pc._opacity, pc._scaling, pc._rotation, None, rs, raw=True)),
        "compensation_torch": lambda: compensation(lambda: compensation_torch(pc._xyz, pc._opacity, pc._scaling, pc._rotation, rs)),
        "filtered": lambda: filtered(lambda: mip.filtered_parameters(pc._scaling, pc._opacity, f)),
        "filtered_torch": lambda: filtered(lambda: filtered_torch(pc._scaling, pc._opacity, f)),
        "filter3d": lambda: mip.filter_3d(pc._xyz, table),
        "filter3d_torch": lambda: filter3d_torch(pc._xyz.detach(), table),
        "step": lambda: step("hip"),
        "step_torch": lambda: step("torch"),
        "step_plain": lambda: step("plain"),
    }
    with torch.no_grad():
        agree = {
            "filter3d_rel": float(((f - f_torch).abs() / f_torch).max()),
            "image_abs": float((step_img("hip", step) - step_img("torch", step)).abs().max()),
        }
    for fn in arms.values():   # warm-up
        fn()
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in arms}
    for _ in range(args.blocks):
        for name, fn in arms.items():
            n = max(1, args.per_block // 5) if name == "filter3d_torch" else args.per_block
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / n)
    med = {k: statistics.median(v) for k, v in ms.items()}
    row = dict(tool="mip_bench", workload=args.workload, P=P, W=W, H=H, cameras=args.cameras, blocks=args.blocks, per_block=args.per_block,
               **{f"{k}_ms": round(v, 4) for k, v in med.items()}, **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
               compensation_bytes=(44 + 4 + 48 + 44) * P, filtered_bytes=(20 + 16 + 36 + 16) * P, filter3d_bytes=(12 + 4 + 4) * P,
               **agree,
               note="events around per_block back-to-back calls (forward and backward for compensation / filtered / step); the per-op "
                    "tensors fit the last-level cache: cache-warm figures; filter3d_torch includes its host loop over the cameras",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    print(json.dumps(row))


def step_img(mode, step):
    with torch.enable_grad():
        return step(mode).detach().clone()


if __name__ == "__main__":
    main()
