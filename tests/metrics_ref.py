"""Float64 restatement of the evaluation metrics (include/r3dgs_metrics.h) for tests/test_metrics_cpu.py and
tests/test_metrics_gpu.py.  Written from the formulas, not imported from the reference tree.

Loading -- the divide by 255, the clamp, the 8-bit rounding -- is done in fp32 exactly as csrc/metrics_math.h specifies;
everything after it in float64.  SSIM is tests/loss_ref's float64 evaluation over the loaded values.  A PSNR is the formula
10 log10(1 / mse) evaluated in float64 with every operation correctly rounded (the logarithm through `decimal`)."""
import decimal
import math

import numpy as np
import torch

from tests import loss_ref

FIELDS = ("l1", "mse", "mse_c0", "mse_c1", "mse_c2", "mse_c3", "psnr_image", "psnr_channels", "ssim")


def quantise8(x):
    """save_image's rounding in fp32: the product rounded, the sum rounded, clamp, truncate; NaN -> 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (x * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    s = np.where(np.isnan(s), np.float32(0.0), s).astype(np.float32)
    return np.clip(s, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def from_u8(u):
    return np.asarray(u, np.uint8).astype(np.float32) / np.float32(255.0)


def clamp01(x):
    x = np.asarray(x, np.float32)
    return np.where(x < 0, np.float32(0.0), np.where(x > 1, np.float32(1.0), x)).astype(np.float32)   # NaN stays NaN


def load_image(image, clamp, quantise):
    """The fp32 values the kernel compares for a float image [C,H,W]."""
    image = np.asarray(image, np.float32)
    if quantise:
        return from_u8(quantise8(image))
    return clamp01(image) if clamp else image


def load_gt(gt, layout, clamp):
    """layout: 'f32' ([C,H,W] float), 'u8_chw' or 'u8_hwc'.  -> fp32 [C,H,W]"""
    if layout == "f32":
        gt = np.asarray(gt, np.float32)
        return clamp01(gt) if clamp else gt
    gt = np.asarray(gt, np.uint8)
    return from_u8(gt if layout == "u8_chw" else np.ascontiguousarray(gt.transpose(2, 0, 1)))


def psnr_db(mse):
    """10 log10(1 / mse) in float64, each operation correctly rounded."""
    mse = float(mse)
    if math.isnan(mse):
        return math.nan
    if mse == 0.0:
        return math.inf
    r = 1.0 / mse
    if math.isinf(r):
        return math.inf
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        lg = float(decimal.Decimal(r).log10())
    return 10.0 * lg


def row(image, gt, layout="f32", clamp=True, quantise=False):
    """-> {field: float} of FIELDS for image [C,H,W] (fp32 values) against gt."""
    x32, y32 = load_image(image, clamp, quantise), load_gt(gt, layout, clamp)
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    C = x.shape[0]
    d = x - y
    mse_c = [float((d[c] * d[c]).mean()) for c in range(C)]
    out = {"l1": float(np.abs(d).mean()), "mse": float((d * d).mean())}
    for c in range(4):
        out[f"mse_c{c}"] = mse_c[c] if c < C else 0.0
    out["psnr_image"] = psnr_db(out["mse"])
    acc = 0.0
    for c in range(C):
        acc += psnr_db(mse_c[c])
    out["psnr_channels"] = acc / C
    if np.isnan(x).any() or np.isnan(y).any():
        out["ssim"] = math.nan
    else:
        w = torch.from_numpy(loss_ref.window32().astype(np.float64))
        m = loss_ref.ssim_map(torch.from_numpy(x[None]), torch.from_numpy(y[None]), w)
        out["ssim"] = float(m.mean())
    return out


def row_mse(a, b):
    """mse of the drop-ins: rows = shape[0], float64 [shape[0]]."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    d = (a - b).reshape(a.shape[0], -1)
    return (d * d).mean(axis=1)


def row_psnr(a, b):
    """20 log10(1 / sqrt(mse)) in float64 per row."""
    return np.array([20.0 * math.log10(1.0 / math.sqrt(m)) if m > 0 else math.inf for m in row_mse(a, b)])
