"""Restatements of the reference's loss (utils/loss_utils.py:17-66, train.py:109-110) for the tests of the fused HIP loss
(tests/test_loss_cpu.py, tests/test_loss_gpu.py).  Written here from the formula, not imported from the reference tree.

evaluate(x, y, dtype) runs the reference's arithmetic with torch on the CPU in `dtype` -- the 11x11 window applied as its
two 1-D factors (the fp32-rounded weights of the reference; a separable evaluation of the same zero-padded convolution) --
and returns values plus the gradient of the requested reduction with respect to x."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window32():
    """The reference's 1-D window: torch.Tensor of the Python doubles (-> fp32), divided by its fp32 sum."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).numpy()


def _filter(t, w):
    """Depthwise zero-padded 11x11 Gaussian filter of t [N,C,H,W] as two 1-D passes."""
    c = t.shape[1]
    wh = w.view(1, 1, 1, 11).expand(c, 1, 1, 11)
    wv = w.view(1, 1, 11, 1).expand(c, 1, 11, 1)
    return F.conv2d(F.conv2d(t, wh, padding=(0, 5), groups=c), wv, padding=(5, 0), groups=c)


def ssim_map(x, y, w):
    mu1, mu2 = _filter(x, w), _filter(y, w)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = _filter(x * x, w) - mu1_sq
    s2 = _filter(y * y, w) - mu2_sq
    s12 = _filter(x * y, w) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def evaluate(x, y, dtype=torch.float64, lam=0.2, upstream=None, per_image_upstream=None):
    """x, y: numpy [B,C,H,W] (or [C,H,W]).  -> dict of
      l1, ssim, loss (= (1-lam) l1 + lam (1-ssim)), ssim_image[B], dloss (d loss / dx),
      and, when given, dmap (d sum(map * upstream) / dx) and dimage (d sum(ssim_image * per_image_upstream) / dx)."""
    shape = x.shape
    x4 = x.reshape((1,) + shape) if x.ndim == 3 else x
    y4 = y.reshape((1,) + shape) if y.ndim == 3 else y
    w = torch.from_numpy(window32().astype(np.float64)).to(dtype)
    xt = torch.from_numpy(np.ascontiguousarray(x4)).to(dtype).requires_grad_()
    yt = torch.from_numpy(np.ascontiguousarray(y4)).to(dtype)
    out = {}
    m = ssim_map(xt, yt, w)
    l1 = (xt - yt).abs().mean()
    s = m.mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    per_image = m.mean(1).mean(1).mean(1)
    out.update(l1=l1.item(), ssim=s.item(), loss=loss.item(), ssim_image=per_image.detach().numpy().astype(np.float64))
    out["dloss"] = torch.autograd.grad(loss, xt, retain_graph=True)[0].numpy().reshape(shape)
    if upstream is not None:
        u = torch.from_numpy(np.ascontiguousarray(upstream.reshape(m.shape))).to(dtype)
        out["dmap"] = torch.autograd.grad((m * u).sum(), xt, retain_graph=True)[0].numpy().reshape(shape)
    if per_image_upstream is not None:
        u = torch.from_numpy(np.ascontiguousarray(per_image_upstream)).to(dtype)
        out["dimage"] = torch.autograd.grad((per_image * u).sum(), xt)[0].numpy().reshape(shape)
    out["map"] = m.detach().numpy().reshape(shape)
    return out


def value_set(name, shape, seed):
    """The three input families of the GPU parity tests: unrelated images in [0,1], a near-identical pair in [0,1], a bright
    near-identical pair with values up to 3."""
    rng = np.random.default_rng(seed)
    if name == "unrelated":
        x, y = rng.random(shape), rng.random(shape)
    elif name == "near":
        x = rng.random(shape)
        y = np.clip(x + rng.normal(0, 0.01, shape), 0, 1)
    elif name == "bright":
        x = 3.0 * rng.random(shape)
        y = np.clip(x + rng.normal(0, 0.01, shape), 0, 3)
    else:
        raise ValueError(name)
    return x.astype(np.float32), y.astype(np.float32)


def torch_formula(img, gt, lam=0.2):
    """The reference's own ops (utils/loss_utils.py:17-66, train.py:109-110) on whatever device img lives on: the 2-D fp32
    window, five depthwise F.conv2d calls with padding 5, autograd for the backward.  -> (loss, Ll1, Lssim)."""
    c = img.size(-3)
    w1 = torch.from_numpy(window32()).to(img.device).unsqueeze(1)
    window = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(c, 1, 11, 11).contiguous()
    mu1 = F.conv2d(img, window, padding=5, groups=c)
    mu2 = F.conv2d(gt, window, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img * img, window, padding=5, groups=c) - mu1_sq
    sigma2_sq = F.conv2d(gt * gt, window, padding=5, groups=c) - mu2_sq
    sigma12 = F.conv2d(img * gt, window, padding=5, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    l1 = torch.abs(img - gt).mean()
    lssim = 1.0 - m.mean()
    return (1.0 - lam) * l1 + lam * lssim, l1, lssim
