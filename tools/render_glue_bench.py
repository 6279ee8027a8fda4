"""What the torch glue between the model and the rasterizer costs, and what the raw-parameter path saves.

    python tools/render_glue_bench.py [--workload metric_500k_1600x1062 train_like_6M_1920x1080] [--steps 20] [--rounds 5]
    python tools/render_glue_bench.py --only A --steps 10      # one form alone, for a rocprofv3 --kernel-trace --stats run

One process, alternating blocks (the scheme of tools/adam_bench.py).  Iteration = render + r3dgs_loss.l1_dssim + backward +
r3dgs_optim.Adam step over the reference's six parameter groups (xyz, f_dc, f_rest, opacity, scaling, rotation):
  A: the reference's glue in torch -- exp(_scaling), F.normalize(_rotation), cat(_features_dc, _features_rest) -- in front
     of the existing rasterizer entry;
  B: the fused path (diff_gaussian_rasterization.rasterize_gaussian_params).
Prints one JSON line per workload: ms per iteration of both (median and every block), the run-to-run spread of the A
blocks, peak allocated memory of both.  Kernel-level numbers come from a separate profiler run of each form (--only)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reduced-3dgs_amd")]
import r3dgs_loss  # noqa: E402
import r3dgs_optim  # noqa: E402
import synth_scene as ss  # noqa: E402

GROUPS = (("xyz", 1.6e-4), ("f_dc", 2.5e-3), ("f_rest", 1.25e-4), ("opacity", 0.05), ("scaling", 5e-3), ("rotation", 1e-3))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def bench(wl, args, dev):
    import diff_gaussian_rasterization as dgr
    w, cam, g = ss.make_workload(wl, seed=0)
    W, H, P = w["W"], w["H"], w["P"]

    def dvt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dvt(np.zeros(3, np.float32)), 1.0,
                                           dvt(cam.world_view_transform), dvt(cam.full_proj_transform), 3,
                                           dvt(cam.camera_center), False, False)
    gt = dvt(np.random.default_rng(1).random((3, H, W)).astype(np.float32))
    degrees = dvt(g["degrees"])
    rng = np.random.default_rng(5)
    raw = dict(xyz=g["means3D"], f_dc=g["sh"][:, :1], f_rest=g["sh"][:, 1:], opacity=g["opacity"],
               scaling=np.log(g["scales"]).astype(np.float32),
               rotation=(g["rotations"] * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32))
    del g
    empty = torch.Tensor([])
    forms = [args.only] if args.only else ["A", "B"]
    leaves = {f: {k: torch.nn.Parameter(dvt(v)) for k, v in raw.items()} for f in forms}
    opts = {f: r3dgs_optim.Adam([{"params": [leaves[f][k]], "lr": lr, "name": k} for k, lr in GROUPS], eps=1e-15) for f in forms}

    def iteration(f):
        p = leaves[f]
        means2D = torch.zeros_like(p["xyz"], requires_grad=True) + 0
        if f == "A":
            color, _ = dgr.rasterize_gaussians(p["xyz"], means2D, torch.cat((p["f_dc"], p["f_rest"]), dim=1), degrees, empty,
                                               p["opacity"], torch.exp(p["scaling"]), F.normalize(p["rotation"]), empty, rs,
                                               0.0)
        else:
            color, _ = dgr.rasterize_gaussian_params(p["xyz"], means2D, p["f_dc"], p["f_rest"], degrees, p["opacity"],
                                                     p["scaling"], p["rotation"], rs, 0.0)
        r3dgs_loss.l1_dssim(color, gt, 0.2)[0].backward()
        opts[f].step()
        opts[f].zero_grad(set_to_none=True)

    for f in forms:
        for _ in range(5):
            iteration(f)
    ms = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            ms[f].append(timed(lambda: iteration(f), args.steps))
    peak = {}
    for f in forms:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        iteration(f)
        torch.cuda.synchronize()
        peak[f] = dict(peak_mb=torch.cuda.max_memory_allocated() / 1e6, above_resident_mb=(torch.cuda.max_memory_allocated() - base) / 1e6)
    out = {"metric": "render_glue", "workload": wl, "gaussians": P, "steps_per_block": args.steps,
           "ms_per_iteration": {f: float(np.median(v)) for f, v in ms.items()}, "ms_all": ms, "memory": peak,
           "joined_sh_tensor_mb": P * 48 * 4 / 1e6}
    if "A" in ms and "B" in ms:
        out["A_spread_ms"] = float(max(ms["A"]) - min(ms["A"]))
        out["saved_ms"] = out["ms_per_iteration"]["A"] - out["ms_per_iteration"]["B"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["metric_500k_1600x1062", "train_like_6M_1920x1080"],
                    choices=list(ss.WORKLOADS))
    ap.add_argument("--steps", type=int, default=20, help="training iterations per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two forms")
    ap.add_argument("--only", choices=["A", "B"], default=None, help="one form only (for a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_glue_bench.py needs a GPU")
    torch.autograd.set_multithreading_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for wl in args.workload:
        bench(wl, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
