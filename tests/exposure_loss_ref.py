"""Float64 restatement of the exposure + mask loss (include/r3dgs_loss.h r3dgs_exposure_loss_*, reduced-3dgs_amd/r3dgs_exposure.py) for
tests/test_exposure_loss_cpu.py and tests/test_exposure_loss_gpu.py.  Written from the formula:

    x'_c  = sum_k E[k,c] x_k + E[c,3]              (the official line: matmul(image.permute(1,2,0), E[:3,:3]).permute(2,0,1) + E[:3,3,None,None])
    x''   = m x'
    y'    = m y if mask_target else y
    loss  = (1 - lam) mean|x'' - y'| + lam (1 - mean SSIM(x'', y'))

with the SSIM of utils/loss_utils.py: the 11-tap window built as the reference builds it (fp32 1-D Gaussian, normalised, its outer
product), five depthwise F.conv2d calls with padding 5.  Gradients come from autograd."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2
# the deliberately wrong exposure the prediction of `inputs` is made with: gains well away from the identity, so that no entry
# of dE is the remainder of a cancellation
WRONG_GAIN = np.array([[0.7, 0.05, 0.0], [0.1, 0.8, -0.05], [0.0, 0.1, 0.9]])
WRONG_OFFSET = 0.1


def window(channels, dtype):
    """utils/loss_utils.py:24-31: create_window(11, channels), the fp32 values carried to `dtype`."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    w1 = (g / g.sum()).unsqueeze(1)
    return w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(channels, 1, 11, 11).contiguous().to(dtype)


def ssim_map(x, y):
    c = x.shape[1]
    w = window(c, x.dtype)
    mu1, mu2 = F.conv2d(x, w, padding=5, groups=c), F.conv2d(y, w, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, w, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(y * y, w, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(x * y, w, padding=5, groups=c) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def exposed(x, E):
    """x [B,3,H,W], E [3,4] or [B,3,4] -> x' by the official line, image by image."""
    Eb = E.expand(x.shape[0], 3, 4) if E.dim() == 2 else E
    return torch.stack([torch.matmul(x[b].permute(1, 2, 0), Eb[b, :3, :3]).permute(2, 0, 1) + Eb[b, :3, 3, None, None]
                        for b in range(x.shape[0])])


def formula(x, y, E=None, m=None, mask_target=False, lam=0.2):
    """torch tensors of one dtype, x and y [B,C,H,W], m broadcastable to them -> (loss, Ll1, Lssim)."""
    if E is not None:
        x = exposed(x, E)
    if m is not None:
        x = x * m
        if mask_target:
            y = y * m
    l1 = (x - y).abs().mean()
    lssim = 1.0 - ssim_map(x, y).mean()
    return (1.0 - lam) * l1 + lam * lssim, l1, lssim


def _mask4(m, B):
    """A mask of any accepted shape ([H,W], [1,H,W], [B,1,H,W]) as [B or 1, 1, H, W]."""
    return None if m is None else m.reshape((-1, 1) + tuple(m.shape[-2:]))


def evaluate(x, y, E=None, m=None, mask_target=False, lam=0.2, dtype=torch.float64):
    """numpy inputs (x, y [3,H,W] or [B,C,H,W]) -> dict(loss, l1, lssim, dx shaped like x, dE shaped like E or None)."""
    shape = x.shape
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape((-1,) + shape[-3:]).requires_grad_()
    yt = torch.from_numpy(np.ascontiguousarray(y)).to(dtype).reshape((-1,) + shape[-3:])
    Et = None if E is None else torch.from_numpy(np.ascontiguousarray(E)).to(dtype).requires_grad_()
    mt = None if m is None else _mask4(torch.from_numpy(np.ascontiguousarray(m)).to(dtype), xt.shape[0])
    loss, l1, lssim = formula(xt, yt, Et, mt, mask_target, lam)
    grads = torch.autograd.grad(loss, [xt] + ([Et] if Et is not None else []))
    return dict(loss=loss.item(), l1=l1.item(), lssim=lssim.item(), dx=grads[0].numpy().reshape(shape),
                dE=grads[1].numpy() if Et is not None else None)


def inputs(shape, seed):
    """-> (x, y, m) float32 for an image shape [3,H,W] or [B,3,H,W]: a smooth target y in [0,1]; the prediction x is the target
    seen through WRONG_GAIN / WRONG_OFFSET plus noise 0.03, clamped to [0,1]; the mask [B or 1 leading dims dropped: H,W per
    image] has about 30 % zeros and the rest in [0.2, 1]."""
    rng = np.random.default_rng(seed)
    B = shape[0] if len(shape) == 4 else 1
    H, W = shape[-2:]
    yy, xx = np.mgrid[0:H, 0:W]
    y = np.empty((B, 3, H, W))
    for b in range(B):
        for c in range(3):
            f = rng.uniform(0.02, 0.12, 4)
            ph = rng.uniform(0, 2 * np.pi, 2)
            y[b, c] = 0.5 + 0.22 * np.sin(f[0] * xx + f[1] * yy + ph[0]) + 0.18 * np.cos(f[2] * xx - f[3] * yy + ph[1])
    y = np.clip(y, 0, 1)
    x = np.einsum("bkhw,kc->bchw", y, WRONG_GAIN) + WRONG_OFFSET + rng.normal(0, 0.03, y.shape)
    x = np.clip(x, 0, 1)
    m = np.where(rng.random((B, 1, H, W)) < 0.3, 0.0, rng.uniform(0.2, 1.0, (B, 1, H, W)))
    return x.astype(np.float32).reshape(shape), y.astype(np.float32).reshape(shape), m.astype(np.float32)


def exposure_guess(B, seed):
    """The exposures the tests evaluate the loss at: [B,3,4] float32 near, not at, the identity."""
    rng = np.random.default_rng(seed)
    E = np.tile(np.eye(3, 4), (B, 1, 1)) + rng.normal(0, 0.08, (B, 3, 4))
    return E.astype(np.float32)
