"""Times the fused exposure + mask loss (reduced-3dgs_amd/r3dgs_exposure.py, the exposure kernels of csrc/loss.hip), forward and
backward, against the same step written as the official torch lines in front of today's r3dgs_loss.l1_dssim, in alternating
blocks, and appends one JSON line to profiles/exposure_loss_bench.jsonl.

    python tools/exposure_loss_bench.py [--height 1062] [--width 1600] [--blocks 6] [--per-block 20]

Per block, each arm a forward + backward with gradients to the image (and to the exposure where there is one):
  * `plain`: r3dgs_loss.l1_dssim(image, gt) alone -- the cost the exposure and the mask are added to;
  * `exposure` / `exposure_torch`, `mask` / `mask_torch`, `both` / `both_torch`: exposed_l1_dssim(...) against
        image = matmul(image.permute(1,2,0), E[:3,:3]).permute(2,0,1) + E[:3,3,None,None];  image = image * mask
    feeding l1_dssim.
Events around per_block back-to-back calls; medians over the blocks, with every block's figure beside them.  The tensors fit the
last-level cache: cache-warm figures.  No speed bar is set.  Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch   # noqa: E402

import r3dgs_exposure   # noqa: E402
import r3dgs_loss   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1062)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_loss_bench.jsonl"))
    args = ap.parse_args()
    H, W = args.height, args.width
    gen = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.rand(3, H, W, device="cuda", generator=gen)
    image = (gt * 0.8 + 0.1 + 0.03 * torch.randn(3, H, W, device="cuda", generator=gen)).clamp(0, 1).requires_grad_()
    mask = (torch.rand(1, H, W, device="cuda", generator=gen) > 0.3).float()
    E = (torch.eye(3, 4, device="cuda") + 0.05 * torch.randn(3, 4, device="cuda", generator=gen)).requires_grad_()

    def torch_lines(use_e, use_m):
        x = image
        if use_e:
            x = torch.matmul(x.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
        if use_m:
            x = x * mask
        return r3dgs_loss.l1_dssim(x, gt)[0]

    def run(loss_fn):
        image.grad = E.grad = None
        loss = loss_fn()
        loss.backward()
        return loss

    arms = {
        "plain": lambda: run(lambda: r3dgs_loss.l1_dssim(image, gt)[0]),
        "exposure": lambda: run(lambda: r3dgs_exposure.exposed_l1_dssim(image, gt, E)[0]),
        "exposure_torch": lambda: run(lambda: torch_lines(True, False)),
        "mask": lambda: run(lambda: r3dgs_exposure.exposed_l1_dssim(image, gt, None, mask)[0]),
        "mask_torch": lambda: run(lambda: torch_lines(False, True)),
        "both": lambda: run(lambda: r3dgs_exposure.exposed_l1_dssim(image, gt, E, mask)[0]),
        "both_torch": lambda: run(lambda: torch_lines(True, True)),
    }
    agree = {}
    for name in ("exposure", "mask", "both"):   # the two routes compute the same step
        a = arms[name]().item()
        ga, ea = image.grad.clone(), None if E.grad is None else E.grad.clone()
        b = arms[name + "_torch"]().item()
        agree[name + "_loss_abs"] = abs(a - b)
        agree[name + "_dimage_rel"] = float((ga - image.grad).abs().max() / image.grad.abs().max())
        if ea is not None:
            agree[name + "_dexposure_rel"] = float((ea - E.grad).abs().max() / E.grad.abs().max())
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
    row = dict(tool="exposure_loss_bench", C=3, H=H, W=W, blocks=args.blocks, per_block=args.per_block,
               **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_speedup": round(med[k + "_torch"] / med[k], 2) for k in ("exposure", "mask", "both")},
               **{f"{k}_over_plain_ms": round(med[k] - med["plain"], 4) for k in ("exposure", "mask", "both")},
               **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()}, **agree,
               note="events around per_block back-to-back forward + backward calls, host launch time included; the tensors fit the "
                    "last-level cache: cache-warm figures",
               library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
