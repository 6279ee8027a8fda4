"""Cost of the training loss of train.py:109-110 on the GPU: the reference's torch formula (utils/loss_utils.py:17-66 -- five
F.conv2d calls, elementwise ops, autograd) against the fused HIP loss (r3dgs_loss.l1_dssim, csrc/loss.hip).  Prints one JSON line.

    python tools/loss_bench.py --workload metric_500k_1600x1062 [--iters 50] [--steps 30] [--only fused|torch]

Measured, for the workload's image size (3 x H x W, seeded target):
  * loss_ms.{torch,fused}: loss forward + backward alone (device events around --iters calls, the two forms alternated in
    blocks of --iters within one process);
  * train_it_s.{torch,fused}: a training iteration -- the render + backward of bench.py's train_step with the loss computed
    from the seeded target instead of the fixed upstream gradient -- in both forms, alternated the same way;
  * fused_bytes / fused_gbps: the fused kernels' compulsory traffic (x, y read twice, the three partial maps written and
    read, the gradient written: 44 B per element) over the event-timed fused loss, against 6.3 TB/s.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/loss_bench.py --only fused` run.
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
from tests import loss_ref  # noqa: E402

HBM_TBS = 6.3
BYTES_PER_ELEMENT = 44   # forward: x, y (8) + partials (12); backward: partials (12) + x, y (8) + gradient (4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="metric_500k_1600x1062", choices=list(ss.WORKLOADS))
    ap.add_argument("--iters", type=int, default=50, help="loss calls per timed block")
    ap.add_argument("--steps", type=int, default=30, help="training iterations per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="alternations torch / fused")
    ap.add_argument("--only", choices=["torch", "fused"], default=None, help="one form only (for a profiler run)")
    ap.add_argument("--lambda-dssim", type=float, default=0.2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench.py needs a GPU")
    torch.autograd.set_multithreading_enabled(False)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lam = args.lambda_dssim

    import diff_gaussian_rasterization as dgr
    w, cam, g = ss.make_workload(args.workload, seed=0)
    W, H = w["W"], w["H"]
    n = 3 * H * W

    def dvt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    leaves = {k: dvt(g[k]).requires_grad_() for k in ("means3D", "opacity", "scales", "rotations", "sh")}
    degrees = dvt(g["degrees"])
    empty = torch.Tensor([])
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dvt(np.zeros(3, np.float32)), 1.0,
                                           dvt(cam.world_view_transform), dvt(cam.full_proj_transform), 3,
                                           dvt(cam.camera_center), False, False)
    gt = dvt(np.random.default_rng(1).random((3, H, W)).astype(np.float32))
    img0 = dvt(np.random.default_rng(2).random((3, H, W)).astype(np.float32))

    forms = {"torch": lambda c, t: loss_ref.torch_formula(c, t, lam), "fused": lambda c, t: r3dgs_loss.l1_dssim(c, t, lam)}
    names = [args.only] if args.only else ["torch", "fused"]

    def loss_only(fn):
        x = img0.detach().requires_grad_()
        fn(x, gt)[0].backward()

    def train_step(fn):
        for t in leaves.values():
            t.grad = None
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
        means2D.retain_grad()
        color, _ = dgr.rasterize_gaussians(leaves["means3D"], means2D, leaves["sh"], degrees, empty, leaves["opacity"],
                                           leaves["scales"], leaves["rotations"], empty, rs, 0.0)
        fn(color, gt)[0].backward()

    def timed(body, fn, count):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(count):
            body(fn)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / count

    for name in names:   # warm-up: code objects, library algorithm choice, the rasterizer's reservation
        for _ in range(5):
            loss_only(forms[name])
            train_step(forms[name])
    loss_ms = {k: [] for k in names}
    step_ms = {k: [] for k in names}
    for _ in range(args.rounds):
        for name in names:
            loss_ms[name].append(timed(loss_only, forms[name], args.iters))
        for name in names:
            step_ms[name].append(timed(train_step, forms[name], args.steps))
    out = {"metric": "loss_fwd_bwd", "workload": args.workload, "image": [3, H, W], "lambda_dssim": lam,
           "loss_ms": {k: float(np.median(v)) for k, v in loss_ms.items()},
           "loss_ms_all": loss_ms,
           "train_it_s": {k: float(1000.0 / np.median(v)) for k, v in step_ms.items()},
           "train_ms_all": step_ms,
           "fused_bytes": BYTES_PER_ELEMENT * n}
    if "fused" in loss_ms:
        t = out["loss_ms"]["fused"] * 1e-3
        out["fused_gbps"] = BYTES_PER_ELEMENT * n / t / 1e9
        out["fused_hbm_bound_us"] = BYTES_PER_ELEMENT * n / (HBM_TBS * 1e12) * 1e6
    if "torch" in loss_ms and "fused" in loss_ms:
        out["loss_speedup"] = out["loss_ms"]["torch"] / out["loss_ms"]["fused"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
