"""`r3dgs_loss` -- the training loss of train.py:109-115 on the MI355X, fused in HIP (csrc/loss.hip, include/r3dgs_loss.h).

    from r3dgs_loss import l1_loss, ssim        # instead of: from utils.loss_utils import l1_loss, ssim
    from r3dgs_loss import l1_dssim             # loss, Ll1, Lssim in one forward launch pair and one backward launch

Same signatures, arithmetic and return shapes as utils/loss_utils.py:17-66 (11-tap Gaussian window, sigma 1.5, zero padding
5, C1 = 0.01^2, C2 = 0.03^2).  Inputs: fp32 device tensors shaped [C,H,W] or [B,C,H,W] (l1_loss: any shape).  Gradients flow
to the first argument only; a differentiable target is refused, as are other window sizes, other dtypes and host tensors
(there is no CPU path).  Values and gradients are deterministic and the calls can be captured in torch.cuda.graph.
"""
import torch

from diff_gaussian_rasterization import _C

__all__ = ["l1_loss", "ssim", "l1_dssim"]

_EMPTY = torch.Tensor([])
_MEAN, _PER_IMAGE, _MAP = 0, 1, 2   # upstream gradient of the SSIM map: of its mean, of the per-image means, of the map


def _check_devices(what, first, **named):
    """Every tensor of `named` that is not None on `first`'s device, which is not the host."""
    for name, t in named.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} is a host tensor; the fused loss needs device tensors (no CPU path)")
        if t.device != first.device:
            raise ValueError(f"{what}: tensors on {first.device} and {t.device}")


def _check_pair(what, a, b, images=True):
    for name, t in (("prediction", a), ("target", b)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} is {t.dtype}; the fused loss takes float32 only")
    if a.shape != b.shape:
        raise ValueError(f"{what}: shapes differ, {tuple(a.shape)} vs {tuple(b.shape)}")
    if images and a.dim() not in (3, 4):
        raise ValueError(f"{what}: expected [C,H,W] or [B,C,H,W], got {tuple(a.shape)}")
    if a.numel() == 0:
        raise ValueError(f"{what}: empty input")
    if b.requires_grad:
        raise RuntimeError(f"{what}: the target requires grad; the fused loss differentiates with respect to the prediction "
                           "only (pass target.detach())")
    _check_devices(what, a, prediction=a, target=b)


def _bchw(t):
    return (1,) + tuple(t.shape) if t.dim() == 3 else tuple(t.shape)


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        x, y = x.contiguous(), y.contiguous()
        ctx.save_for_backward(x, y)
        return _C.l1_forward(x, y)

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        return _C.l1_backward(x, y, g.contiguous()), None


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, mode):
        shape = img1.shape
        B, C, H, W = _bchw(img1)
        x, y = img1.contiguous(), img2.contiguous()
        train = ctx.needs_input_grad[0]
        _, s_mean, _, _, s_img, s_map, partials = _C.l1_ssim_forward(x, y, B, C, H, W, 0.0, train, mode == _MAP)
        ctx.dims, ctx.mode = (B, C, H, W), mode
        if train:
            ctx.save_for_backward(x, y, partials)
        if mode == _MAP:
            return s_map.view(shape)
        return s_img if mode == _PER_IMAGE else s_mean

    @staticmethod
    def backward(ctx, g):
        x, y, partials = ctx.saved_tensors
        B, C, H, W = ctx.dims
        dx = _C.l1_ssim_backward(x, y, partials, _EMPTY, 0.0, g.contiguous(), ctx.mode, 1.0, B, C, H, W)
        return dx.view(x.shape), None, None


class _L1DSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lam):
        B, C, H, W = _bchw(image)
        x, y = image.contiguous(), gt.contiguous()
        train = ctx.needs_input_grad[0]
        l1, _, loss, dssim, _, _, partials = _C.l1_ssim_forward(x, y, B, C, H, W, lam, train, False)
        ctx.dims, ctx.lam = (B, C, H, W), lam
        if train:
            ctx.save_for_backward(x, y, partials)
        ctx.mark_non_differentiable(l1, dssim)
        return loss, l1, dssim

    @staticmethod
    def backward(ctx, g_loss, _g_l1, _g_dssim):
        x, y, partials = ctx.saved_tensors
        B, C, H, W = ctx.dims
        g = g_loss.contiguous()
        # loss = (1 - lam) L1 + lam (1 - S): upstream of the L1 mean (1 - lam) g, of the SSIM mean -lam g
        dx = _C.l1_ssim_backward(x, y, partials, g, 1.0 - ctx.lam, g, _MEAN, -ctx.lam, B, C, H, W)
        return dx.view(x.shape), None, None


def l1_loss(network_output, gt):
    """utils/loss_utils.py:17-18: mean |network_output - gt| (0-d), any shape; gradient to network_output."""
    _check_pair("l1_loss", network_output, gt, images=False)
    return _L1.apply(network_output, gt)


def ssim(img1, img2, window_size=11, size_average=True, aggregate=True):
    """utils/loss_utils.py:33-47: mean SSIM (0-d), per-image mean SSIM ([B], size_average=False, 4-D input) or the SSIM
    map (aggregate=False, img1's shape); gradient to img1."""
    if window_size != 11:
        raise ValueError(f"ssim: window_size={window_size}; the fused kernel implements the reference's 11-tap window only")
    if aggregate and not size_average and isinstance(img1, torch.Tensor) and img1.dim() != 4:
        raise ValueError("ssim: size_average=False needs [B,C,H,W] input (the reference's three .mean(1) need 4-D)")
    _check_pair("ssim", img1, img2)
    mode = _MAP if not aggregate else (_MEAN if size_average else _PER_IMAGE)
    return _SSIM.apply(img1, img2, mode)


def l1_dssim(image, gt, lambda_dssim=0.2):
    """train.py:109-110 in one forward launch pair and one backward launch:
    -> (loss, Ll1, Lssim) with loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * Lssim, Lssim = 1 - SSIM(image, gt).
    Only `loss` carries a gradient (to image)."""
    _check_pair("l1_dssim", image, gt)
    return _L1DSSIM.apply(image, gt, float(lambda_dssim))
