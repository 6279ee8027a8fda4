"""Cost of the visibility-masked bookkeeping of a training iteration (train.py:105-106, :113, :134,
scene/gaussian_model.py:693-695): the reference's torch lines (boolean-mask indexing: every x[mask] runs nonzero, a host
wait) against the three HIP calls of r3dgs_train_stats (csrc/train_stats.hip), on synth_scene workloads.  One JSON line per
workload, appended to --out (default profiles/train_stats_bench.jsonl).

    python tools/train_stats_bench.py [--workload metric_500k_1600x1062 ...] [--iters 50] [--steps 20] [--rounds 3] [--out FILE]

Both sides run in one process, alternated in blocks, after a warm-up of every shape and form.  Measured per workload:
  * stats_ms.{torch,hip}: the statistics alone on the tensors a real render + backward left -- the two means, the backward of
    lambda * Lalpha_regul into opacity.grad, the three accumulator updates -- timed with device events around --iters
    repetitions (median of --rounds blocks).  The torch side's host waits are inside the window, as they are in training;
  * visible_means_ms: the visible_means call alone, event-timed, against its roof: visible rows x 12 (M - 1) + 8 P bytes over
    6.3 TB/s (roof_ms, roof_fraction);
  * train_ms.{torch,hip} / train_wall_ms.{torch,hip}: a full iteration -- render, r3dgs_loss.l1_dssim + lambda * Lalpha_regul,
    backward, the statistics, r3dgs_optim.Adam step -- per iteration, event-timed and by the host clock around --steps
    iterations ending in a synchronise.
The GPU is required; there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth_scene as ss  # noqa: E402
import r3dgs_loss  # noqa: E402
import r3dgs_optim  # noqa: E402
import r3dgs_train_stats as ts  # noqa: E402
from tests import trainstats_ref  # noqa: E402

HBM_TBS = 6.3
LAMBDA_ALPHA, LAMBDA_SH = 0.01, 0.05
FORMS = ("torch", "hip")


class Model:
    """The reference GaussianModel's raw parameters and densification accumulators."""

    def __init__(self, g, dev):
        def dvt(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        P = g["means3D"].shape[0]
        self._xyz = torch.nn.Parameter(dvt(g["means3D"]))
        self._features_dc = torch.nn.Parameter(dvt(g["sh"][:, :1]))
        self._features_rest = torch.nn.Parameter(dvt(g["sh"][:, 1:]))
        self._opacity = torch.nn.Parameter(dvt(g["opacity"]))
        self._scaling = torch.nn.Parameter(torch.log(dvt(g["scales"])))
        self._rotation = torch.nn.Parameter(dvt(g["rotations"]))
        self.degrees = dvt(g["degrees"])
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self.max_radii2D = torch.zeros(P, device=dev)

    def params(self):
        return [self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation]


def means_torch(pc, radii):
    vis = radii > 0
    Lalpha = torch.sigmoid(pc._opacity)[vis].abs().mean()                                     # train.py:105-106
    sh = LAMBDA_SH * pc._features_rest.detach()[vis].abs().mean()                             # train.py:113
    return vis, Lalpha, sh


def densify_torch(pc, vis, radii, viewspace_grad):
    pc.max_radii2D[vis] = torch.max(pc.max_radii2D[vis], radii[vis])                          # train.py:134
    pc.xyz_gradient_accum += torch.norm(viewspace_grad[:, :2], dim=-1, keepdim=True)          # gaussian_model.py:694
    pc.denom += vis.unsqueeze(1)                                                              # gaussian_model.py:695


def means_hip(pc, radii):
    vm = ts.visible_means(radii, opacity=pc._opacity, features_rest=pc._features_rest)
    return vm.visibility_filter, vm.alpha_mean, LAMBDA_SH * vm.sh_abs_mean


def densify_hip(pc, vis, radii, viewspace_grad):
    ts.add_densification_stats(pc, viewspace_grad, radii)


MEANS = {"torch": means_torch, "hip": means_hip}
DENSIFY = {"torch": densify_torch, "hip": densify_hip}


def timed(body, count):
    """-> (event ms, host-clock ms) per repetition; the host clock stops after the synchronise."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(count):
        body()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / count, (time.perf_counter() - t0) * 1e3 / count


def render(dgr, rs, pc):
    means2D = torch.zeros_like(pc._xyz, requires_grad=True) + 0
    means2D.retain_grad()
    color, radii = dgr.GaussianRasterizer(rs)(
        means3D=pc._xyz, means2D=means2D, shs=torch.cat([pc._features_dc, pc._features_rest], 1), degrees=pc.degrees,
        colors_precomp=None, opacities=torch.sigmoid(pc._opacity), scales=torch.exp(pc._scaling),
        rotations=torch.nn.functional.normalize(pc._rotation), cov3D_precomp=None, lambda_sh_sparsity=0.0)
    return color, radii, means2D


def bench(wl, args, dev):
    import diff_gaussian_rasterization as dgr

    w, cam, g = ss.make_workload(wl, seed=0)
    P, W, H = w["P"], w["W"], w["H"]
    pc = Model(g, dev)
    M = pc._features_rest.shape[1] + 1

    def dvt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dvt(np.zeros(3, np.float32)), 1.0,
                                           dvt(cam.world_view_transform), dvt(cam.full_proj_transform), 3,
                                           dvt(cam.camera_center), False, False)
    gt = dvt(np.random.default_rng(1).random((3, H, W)).astype(np.float32))
    lrs = (0.00016, 0.0025, 0.000125, 0.05, 0.005, 0.001)
    opt = r3dgs_optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(pc.params(), lrs)], lr=0.0, eps=1e-15)

    def iteration(form):
        color, radii, means2D = render(dgr, rs, pc)
        vis, Lalpha, _sh = MEANS[form](pc, radii)
        loss = r3dgs_loss.l1_dssim(color, gt, 0.2)[0] + LAMBDA_ALPHA * Lalpha
        loss.backward()
        with torch.no_grad():
            DENSIFY[form](pc, vis, radii, means2D.grad)
        opt.step()
        opt.zero_grad(set_to_none=True)

    # the tensors a render + backward leaves, for the statistics alone
    color, radii, means2D = render(dgr, rs, pc)
    r3dgs_loss.l1_dssim(color, gt, 0.2)[0].backward()
    radii, vg = radii.clone(), means2D.grad.clone()
    opt.zero_grad(set_to_none=True)
    n_visible = int((radii > 0).sum())

    def stats_alone(form):
        vis, Lalpha, _sh = MEANS[form](pc, radii)
        (LAMBDA_ALPHA * Lalpha).backward()
        with torch.no_grad():
            DENSIFY[form](pc, vis, radii, vg)

    def means_alone():
        ts.visible_means(radii, opacity=pc._opacity.detach(), features_rest=pc._features_rest)

    for form in FORMS:   # warm-up of every form at this shape: code objects, allocator, graphs, clocks
        for _ in range(5):
            iteration(form)
        for _ in range(10):
            stats_alone(form)
    for _ in range(10):
        means_alone()
    stats_ms, train_ms, train_wall = ({k: [] for k in FORMS} for _ in range(3))
    vm_ms = []
    for _ in range(args.rounds):
        for form in FORMS:
            stats_ms[form].append(timed(lambda: stats_alone(form), args.iters)[0])
        vm_ms.append(timed(means_alone, args.iters)[0])
        for form in FORMS:
            ev, wall = timed(lambda: iteration(form), args.steps)
            train_ms[form].append(ev)
            train_wall[form].append(wall)
    med = lambda d: {k: float(np.median(v)) for k, v in d.items()}   # noqa: E731
    vm_bytes = trainstats_ref.visible_means_bytes(P, M, n_visible)
    roof_ms = vm_bytes / (HBM_TBS * 1e12) * 1e3
    out = {"metric": "train_stats", "workload": wl, "gaussians": P, "width": W, "height": H, "visible": n_visible,
           "stats_ms": med(stats_ms), "stats_ms_all": stats_ms,
           "visible_means_ms": float(np.median(vm_ms)), "visible_means_bytes": vm_bytes, "roof_ms": roof_ms,
           "roof_fraction": roof_ms / float(np.median(vm_ms)),
           "train_ms": med(train_ms), "train_ms_all": train_ms, "train_wall_ms": med(train_wall), "train_wall_ms_all": train_wall,
           "iters": args.iters, "steps": args.steps, "rounds": args.rounds}
    out["stats_speedup"] = out["stats_ms"]["torch"] / out["stats_ms"]["hip"]
    out["train_wall_speedup"] = out["train_wall_ms"]["torch"] / out["train_wall_ms"]["hip"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["metric_500k_1600x1062", "garden_like_2M_1600x1062",
                                                      "train_like_6M_1920x1080"], choices=list(ss.WORKLOADS))
    ap.add_argument("--iters", type=int, default=50, help="repetitions of the statistics per timed block")
    ap.add_argument("--steps", type=int, default=20, help="training iterations per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_stats_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_stats_bench.py needs a GPU")
    torch.autograd.set_multithreading_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for wl in args.workload:
        line = json.dumps(bench(wl, args, dev))
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
