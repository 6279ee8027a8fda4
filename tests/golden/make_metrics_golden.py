"""Writes tests/golden/ref_metrics.npz, the fixture of tests/test_metrics_cpu.py / test_metrics_gpu.py: the reference's own
psnr / mse (utils/image_utils.py), l1_loss / ssim (utils/loss_utils.py) and torch's CPU result of save_image's 8-bit
rounding, on one seeded 3x40x56 image with values in [-0.2, 1.3] and a ground truth in [0, 1].

    python tests/golden/make_metrics_golden.py /path/to/reference

Runs on the CPU.  Only the inputs and the recorded results are written: data of the reference's programs, none of their text."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    sys.path.insert(0, ref)
    from utils.image_utils import mse, psnr
    from utils.loss_utils import l1_loss, ssim
    g = torch.Generator().manual_seed(17)
    image = torch.rand(3, 40, 56, generator=g) * 1.5 - 0.2
    gt = torch.rand(3, 40, 56, generator=g)
    ci, cg = torch.clamp(image, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)   # train.py:256-257
    out = dict(
        image=image.numpy(), gt=gt.numpy(),
        # train.py:263: the [3,H,W] form, rows = channels
        psnr_chw=psnr(ci, cg).numpy(), mse_chw=mse(ci, cg).numpy(),
        # metrics.py:73: the [1,3,H,W] form, one row
        psnr_bchw=psnr(ci[None], cg[None]).numpy(), mse_bchw=mse(ci[None], cg[None]).numpy(),
        # the same on the images as they are (the drop-ins do not clamp)
        psnr_raw_chw=psnr(image, gt).numpy(), mse_raw_chw=mse(image, gt).numpy(),
        l1=np.float32(l1_loss(ci, cg).item()), ssim=np.float32(ssim(ci, cg).item()),
        # torchvision.utils.save_image's conversion (render.py writes its PNGs through it), CHW as torch computes it
        bytes_chw=image.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy())
    path = os.path.join(HERE, "ref_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
