"""Cost of judging one view on the GPU at 3x1062x1600 (train.py:253-265; metrics.py:71-73): the reference's torch lines
against the fused r3dgs_metrics.image_metrics (csrc/metrics.hip), and the nearest form the library had before it.

    python tools/metrics_bench.py [--iters 50] [--rounds 3] [--out profiles/metrics_bench.jsonl] [--reference /path/to/reference]

Four legs alternate in blocks of --iters calls within one process, --rounds times after a warm-up, each block between device
events:
  torch         the reference's lines: clamp x2, l1_loss, psnr, and the torch-formula ssim (five depthwise convolutions) --
                the reference's own functions when --reference (or a checkout on sys.path) provides utils/, otherwise
                tests/loss_ref.torch_formula, the same fp32 formula
  fused_f32     image_metrics with a float ground truth            (8 B per element read)
  fused_u8      image_metrics with a uint8 [H,W,C] ground truth    (5 B per element read)
  loss_ssim     r3dgs_loss.ssim under no_grad: the parent's nearest form (no clamp, no squared error, no 8-bit truth)
One JSON line, printed and appended to --out: the medians, every block, loss_ssim's own min-to-max spread over the blocks,
and whether the medians of the fused legs are within loss_ssim's median plus that spread (DESIGN.md 15's convention).
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

import r3dgs_loss  # noqa: E402
import r3dgs_metrics  # noqa: E402
from tests import loss_ref  # noqa: E402

SHAPE = (3, 1062, 1600)
HBM_TBS = 6.3


def timed(body, count):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        body()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / count


def torch_leg(reference):
    """The reference's evaluation lines as a callable of (image, gt) and where its functions came from."""
    if reference:
        sys.path.insert(0, reference)
    try:
        from utils.image_utils import psnr
        from utils.loss_utils import l1_loss, ssim
        source = "reference checkout"
    except ImportError:
        source = "tests/loss_ref.torch_formula"

        def psnr(a, b):
            return 20 * torch.log10(1.0 / torch.sqrt(((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)))

        def l1_loss(a, b):
            return torch.abs(a - b).mean()

        def ssim(a, b):
            return 1.0 - loss_ref.torch_formula(a, b)[2]

    def body(image, gt):
        x, y = torch.clamp(image, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)
        return l1_loss(x, y).mean().double(), psnr(x, y).mean().double(), ssim(x[None], y[None])
    return body, source


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.jsonl"))
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py needs a GPU")
    rng = np.random.default_rng(0)
    image = torch.from_numpy(rng.uniform(-0.2, 1.3, SHAPE).astype(np.float32)).cuda()
    gt_u8 = torch.from_numpy(rng.integers(0, 256, (SHAPE[1], SHAPE[2], SHAPE[0]), dtype=np.uint8)).cuda()
    gt_f32 = (gt_u8.permute(2, 0, 1).float() / 255).contiguous()
    row = torch.empty(r3dgs_metrics.ROW, dtype=torch.float64, device="cuda")
    torch_body, source = torch_leg(args.reference)
    with torch.no_grad():
        legs = {"torch": lambda: torch_body(image, gt_f32),
                "fused_f32": lambda: r3dgs_metrics.image_metrics(image, gt_f32, out=row),
                "fused_u8": lambda: r3dgs_metrics.image_metrics(image, gt_u8, out=row),
                "loss_ssim": lambda: r3dgs_loss.ssim(image, gt_f32)}
        for body in legs.values():   # warm-up: code objects, MIOpen's algorithm search, the allocator's blocks
            timed(body, 5)
        blocks = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, body in legs.items():
                blocks[k].append(timed(body, args.iters))
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    spread = max(blocks["loss_ssim"]) - min(blocks["loss_ssim"])
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    out = {"tool": "metrics_bench", "shape": list(SHAPE), "iters": args.iters, "rounds": args.rounds, "torch_leg": source,
           "device": torch.cuda.get_device_name(0), "call_ms": med, "blocks_ms": blocks, "loss_ssim_spread_ms": spread,
           "bar_ms": med["loss_ssim"] + spread,
           "within_bar": {k: med[k] <= med["loss_ssim"] + spread for k in ("fused_f32", "fused_u8")},
           "bytes_per_element": {"fused_f32": 8, "fused_u8": 5},
           "call_bytes_over_hbm_peak": {k: b * n / (med[k] * 1e-3) / (HBM_TBS * 1e12) for k, b in (("fused_f32", 8), ("fused_u8", 5))}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
