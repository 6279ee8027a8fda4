"""Cost of the optimizer step of train.py:154 on the GPU: torch.optim.Adam (the reference's default foreach step),
torch.optim.Adam(fused=True) and the fused HIP step r3dgs_optim.Adam (csrc/optim.hip), on the reference's six parameter groups
(scene/gaussian_model.py:210-217: xyz, f_dc, f_rest, opacity, scaling, rotation; degree 3, 59 floats per Gaussian) at a
synth_scene workload's Gaussian count.  Prints one JSON line per workload.

    python tools/adam_bench.py [--workload metric_500k_1600x1062 ...] [--iters 50] [--steps 20] [--only hip|foreach|fused]
                               [--no-train]
    python tools/adam_bench.py --visible [--visible-out profiles/visible_adam_bench.jsonl] [--workload ...] [--iters 50]

Measured per workload:
  * step_ms.{foreach,fused,hip}: one optimizer step (device events around --iters steps; the three forms alternated in
    blocks of --iters within one process, --rounds times; medians);
  * hip_tbs: 28 B per parameter (read p, g, m, v; write p, m, v) over the event-timed HIP step, against 6.3 TB/s;
  * train_it_s.{foreach,fused,hip}: a training iteration -- render + backward of bench.py's train_step with the loss
    r3dgs_loss.l1_dssim against a seeded target, then the optimizer step over the rasterizer's five leaves -- alternated the
    same way.
With --visible the legs of the visibility-gated step run instead (r3dgs_optim.Adam.step(radii=...)): per workload's Gaussian
count, visible fractions 1.0, 0.5 and 0.25, each drawn independently per Gaussian and in runs of 64 consecutive Gaussians;
the dense and the gated step of one optimizer alternate in blocks of --iters within the process, --rounds times.  One JSON
line per leg, printed and appended to --visible-out: the medians, every block, the dense step's own spread over the
alternations, and the byte estimate dense * (1 - 0.76 (1 - fraction)) of DESIGN.md 13.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/adam_bench.py --only hip --no-train` run.
The GPU is required; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth_scene as ss  # noqa: E402
import r3dgs_loss  # noqa: E402
import r3dgs_optim  # noqa: E402
from tests import adam_ref  # noqa: E402

HBM_TBS = 6.3
BYTES_PER_PARAM = 28   # read p, g, m, v; write p, m, v
FORMS = {"foreach": lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15),
         "fused": lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True),
         "hip": lambda groups: r3dgs_optim.Adam(groups, lr=0.0, eps=1e-15)}


def timed(body, count):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        body()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / count


def step_bench(P, names, args, dev):
    """Optimizer step alone on the six reference groups at P Gaussians (fixed random gradients)."""
    gen = torch.Generator(device=dev).manual_seed(0)
    opts = {}
    for name in names:
        params = [torch.nn.Parameter(torch.randn((P,) + shape, device=dev, generator=gen)) for _, shape, _ in adam_ref.GROUPS]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        opts[name] = FORMS[name]([{"params": [p], "lr": lr, "name": n} for p, (n, _, lr) in zip(params, adam_ref.GROUPS)])
    n_params = P * sum(int(np.prod(s)) for _, s, _ in adam_ref.GROUPS)
    for name in names:
        for _ in range(5):
            opts[name].step()
    ms = {k: [] for k in names}
    for _ in range(args.rounds):
        for name in names:
            ms[name].append(timed(opts[name].step, args.iters))
    del opts
    torch.cuda.empty_cache()
    return n_params, ms


VISIBLE_FRACTIONS = (1.0, 0.5, 0.25)
VISIBLE_PATTERNS = {"independent": 1, "runs64": 64}   # Gaussians per run that share one draw
REST_SHARE = 0.76   # f_rest's 45 of the 59 floats: rows long enough that a culled row's lines are skipped whole


def visible_radii(P, fraction, run, gen, dev):
    draws = torch.rand((P + run - 1) // run, device=dev, generator=gen) < fraction
    return torch.where(draws.repeat_interleave(run)[:P], 7, 0).to(torch.int32).contiguous()


def visible_bench(P, args, dev):
    """The gated step against the dense one on the six reference groups at P Gaussians: yields one leg per fraction and
    pattern.  Both forms step the same optimizer (fixed random gradients), alternating in blocks of --iters."""
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(torch.randn((P,) + shape, device=dev, generator=gen)) for _, shape, _ in adam_ref.GROUPS]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    opt = FORMS["hip"]([{"params": [p], "lr": lr, "name": n} for p, (n, _, lr) in zip(params, adam_ref.GROUPS)])
    n_params = sum(p.numel() for p in params)
    for fraction in VISIBLE_FRACTIONS:
        for pattern, run in VISIBLE_PATTERNS.items():
            radii = visible_radii(P, fraction, run, gen, dev)
            forms = {"dense": opt.step, "gated": lambda: opt.step(radii=radii)}
            for body in forms.values():
                for _ in range(5):
                    body()
            ms = {k: [] for k in forms}
            for _ in range(args.rounds):
                for name, body in forms.items():
                    ms[name].append(timed(body, args.iters))
            dense, gated = (float(np.median(ms[k])) for k in ("dense", "gated"))
            yield {"metric": "adam_step_visible", "gaussians": P, "params": n_params, "fraction": fraction,
                   "pattern": pattern, "visible": int((radii > 0).sum()) / P, "step_ms": {"dense": dense, "gated": gated},
                   "step_ms_all": ms, "dense_spread_ms": float(max(ms["dense"]) - min(ms["dense"])),
                   "gated_over_dense": gated / dense, "byte_estimate_ms": dense * (1 - REST_SHARE * (1 - fraction)),
                   "iters": args.iters, "rounds": args.rounds}


def train_bench(w, cam, g, names, args, dev):
    import diff_gaussian_rasterization as dgr

    def dvt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    W, H = w["W"], w["H"]
    degrees = dvt(g["degrees"])
    empty = torch.Tensor([])
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dvt(np.zeros(3, np.float32)), 1.0,
                                           dvt(cam.world_view_transform), dvt(cam.full_proj_transform), 3,
                                           dvt(cam.camera_center), False, False)
    gt = dvt(np.random.default_rng(1).random((3, H, W)).astype(np.float32))
    keys = ("means3D", "opacity", "scales", "rotations", "sh")
    lrs = (0.00016, 0.05, 0.005, 0.001, 0.0025)
    leaves = {k: torch.nn.Parameter(dvt(g[k])) for k in keys}
    opts = {name: FORMS[name]([{"params": [leaves[k]], "lr": lr} for k, lr in zip(keys, lrs)]) for name in names}

    def iteration(opt):
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
        color, _ = dgr.rasterize_gaussians(leaves["means3D"], means2D, leaves["sh"], degrees, empty, leaves["opacity"],
                                           leaves["scales"], leaves["rotations"], empty, rs, 0.0)
        r3dgs_loss.l1_dssim(color, gt, 0.2)[0].backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    for name in names:
        for _ in range(5):
            iteration(opts[name])
    ms = {k: [] for k in names}
    for _ in range(args.rounds):
        for name in names:
            ms[name].append(timed(lambda: iteration(opts[name]), args.steps))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["metric_500k_1600x1062", "train_like_6M_1920x1080"],
                    choices=list(ss.WORKLOADS))
    ap.add_argument("--iters", type=int, default=50, help="optimizer steps per timed block")
    ap.add_argument("--steps", type=int, default=20, help="training iterations per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms")
    ap.add_argument("--only", choices=list(FORMS), default=None, help="one form only (for a profiler run)")
    ap.add_argument("--no-train", action="store_true", help="optimizer steps only")
    ap.add_argument("--visible", action="store_true", help="the legs of the visibility-gated step instead")
    ap.add_argument("--visible-out", default=os.path.join(ROOT, "profiles", "visible_adam_bench.jsonl"),
                    help="with --visible: the file each leg's JSON line is appended to")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench.py needs a GPU")
    torch.autograd.set_multithreading_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    names = [args.only] if args.only else list(FORMS)
    if args.visible:
        with open(args.visible_out, "a") as f:
            for wl in args.workload:
                for leg in visible_bench(ss.WORKLOADS[wl]["P"], args, dev):
                    line = json.dumps({"workload": wl, **leg})
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                torch.cuda.empty_cache()
        return
    for wl in args.workload:
        w, cam, g = ss.make_workload(wl, seed=0)
        P = w["P"]
        n_params, step_ms = step_bench(P, names, args, dev)
        out = {"metric": "adam_step", "workload": wl, "gaussians": P, "params": n_params,
               "step_ms": {k: float(np.median(v)) for k, v in step_ms.items()}, "step_ms_all": step_ms,
               "hip_bytes": BYTES_PER_PARAM * n_params,
               "hbm_bound_ms": BYTES_PER_PARAM * n_params / (HBM_TBS * 1e12) * 1e3}
        if "hip" in step_ms:
            out["hip_tbs"] = BYTES_PER_PARAM * n_params / (out["step_ms"]["hip"] * 1e-3) / 1e12
            for other in ("foreach", "fused"):
                if other in step_ms:
                    out[f"speedup_vs_{other}"] = out["step_ms"][other] / out["step_ms"]["hip"]
        if not args.no_train:
            train_ms = train_bench(w, cam, g, names, args, dev)
            out["train_it_s"] = {k: float(1000.0 / np.median(v)) for k, v in train_ms.items()}
            out["train_ms_all"] = train_ms
        print(json.dumps(out), flush=True)
        del g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
