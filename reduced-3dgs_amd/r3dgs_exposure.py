"""`r3dgs_exposure` -- the training loss of r3dgs_loss.l1_dssim behind a per-image exposure and a pixel mask, fused in HIP
(csrc/loss.hip's exposure kernels, csrc/exposure_math.h, include/r3dgs_loss.h).

    from r3dgs_exposure import ExposureTable, exposed_l1_dssim, apply_exposure
    exposures = ExposureTable(len(train_cameras)).cuda()                   # one learnable 3 x 4 colour map per training image
    loss, Ll1, Lssim = exposed_l1_dssim(image, gt, exposures[cam.uid], mask=cam.alpha_mask)
    shown = apply_exposure(image, exposures[cam.uid], clamp=True)          # evaluation / saving (train_test_exp)

The official 3DGS train.py (Oct 2024) writes this as torch lines in front of its loss,
    image = torch.matmul(image.permute(1, 2, 0), exposure[:3, :3]).permute(2, 0, 1) + exposure[:3, 3, None, None]
    image *= alpha_mask
which costs about a dozen full-image passes per step and autograd's copies of them.  Here the map runs inside the loss's tile
kernels: x'_c = sum_k E[k,c] x_k + E[c,3], x'' = m x', y' = m y (mask_target=True) or y, and
loss = (1 - lambda) mean|x'' - y'| + lambda (1 - mean SSIM(x'', y')), the means over all elements (no renormalisation by the mask's
area).  Gradients flow to the image and to the exposure; a target or a mask that requires grad is refused.  Inputs are float32
device tensors (no CPU path).  Values and gradients are deterministic and the calls can be captured in torch.cuda.graph.
"""
import torch

from diff_gaussian_rasterization import _C
from r3dgs_loss import _bchw, _check_devices, _check_pair

__all__ = ["exposed_l1_dssim", "apply_exposure", "ExposureTable"]


def _check_exposure(what, exposure, image):
    """-> per_image: whether `exposure` is [B,3,4] (one map per image of the batch) rather than one [3,4]."""
    if not isinstance(exposure, torch.Tensor):
        raise TypeError(f"{what}: exposure must be a tensor")
    if exposure.dtype != torch.float32:
        raise TypeError(f"{what}: exposure is {exposure.dtype}; the fused loss takes float32 only")
    B, C = _bchw(image)[:2]
    if C != 3:
        raise ValueError(f"{what}: an exposure maps 3 colour channels, the image has C = {C}")
    if tuple(exposure.shape) not in ((3, 4), (B, 3, 4)):
        raise ValueError(f"{what}: expected an exposure of shape (3, 4) or ({B}, 3, 4), got {tuple(exposure.shape)}")
    return exposure.dim() == 3


def _check_mask(what, mask, image):
    """-> per_image: whether `mask` is [B,1,H,W] rather than one [H,W] / [1,H,W] shared by the batch."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{what}: mask must be a tensor")
    if mask.dtype != torch.float32:
        raise TypeError(f"{what}: mask is {mask.dtype}; the fused loss takes float32 only (mask.float())")
    B, _, H, W = _bchw(image)
    if tuple(mask.shape) not in ((H, W), (1, H, W), (B, 1, H, W)):
        raise ValueError(f"{what}: expected a mask of shape ({H}, {W}), (1, {H}, {W}) or ({B}, 1, {H}, {W}), got {tuple(mask.shape)}")
    if mask.requires_grad:
        raise RuntimeError(f"{what}: the mask requires grad; the fused loss differentiates with respect to the prediction and the "
                           "exposure only (pass mask.detach())")
    return mask.dim() == 4


def _check_image(what, image):
    """What _bchw needs of the prediction, before the exposure and the mask are held against it."""
    if not isinstance(image, torch.Tensor):
        raise TypeError(f"{what}: prediction must be a tensor")
    if image.dim() not in (3, 4) or image.numel() == 0:
        raise ValueError(f"{what}: expected [C,H,W] or [B,C,H,W], got {tuple(image.shape)}")


class _ExposedL1DSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, exposure, mask, flags, lam):
        e_per_image, m_per_image, mask_target = flags
        B, C, H, W = _bchw(image)
        x, y = image.contiguous(), gt.contiguous()
        E = None if exposure is None else exposure.contiguous()
        m = None if mask is None else mask.contiguous()
        train = ctx.needs_input_grad[0] or ctx.needs_input_grad[2]
        l1, _, loss, dssim, _, partials = _C.exposure_loss_forward(x, y, E, e_per_image, m, m_per_image, mask_target, B, C, H, W,
                                                                   lam, train)
        ctx.dims, ctx.lam, ctx.flags = (B, C, H, W), lam, flags
        ctx.has = (E is not None, m is not None)
        if train:
            ctx.save_for_backward(x, y, partials, *(t for t in (E, m) if t is not None))
        ctx.mark_non_differentiable(l1, dssim)
        return loss, l1, dssim

    @staticmethod
    def backward(ctx, g_loss, _g_l1, _g_dssim):
        x, y, partials, *rest = ctx.saved_tensors
        E = rest.pop(0) if ctx.has[0] else None
        m = rest.pop(0) if ctx.has[1] else None
        B, C, H, W = ctx.dims
        e_per_image, m_per_image, mask_target = ctx.flags
        want_dE = E is not None and ctx.needs_input_grad[2]
        # loss = (1 - lam) L1 + lam (1 - S): upstream of the L1 mean (1 - lam) g, of the SSIM mean -lam g
        dx, dE = _C.exposure_loss_backward(x, y, E, e_per_image, m, m_per_image, mask_target, partials, g_loss.contiguous(),
                                           1.0 - ctx.lam, -ctx.lam, want_dE, B, C, H, W)
        return (dx.view(x.shape) if ctx.needs_input_grad[0] else None, None, dE.view(E.shape) if want_dE else None, None, None,
                None)


def exposed_l1_dssim(image, gt, exposure=None, mask=None, mask_target=False, lambda_dssim=0.2):
    """train.py's loss with its exposure and mask lines folded in -> (loss, Ll1, Lssim), loss = (1 - lambda_dssim) * Ll1 +
    lambda_dssim * Lssim of (m (image E[:, :3] + E[:, 3]), mask_target ? m gt : gt).  Only `loss` carries a gradient (to image
    and to exposure).
      image, gt   [3,H,W] or [B,3,H,W] (any C >= 1 without an exposure)
      exposure    [3,4], or [B,3,4] for one map per image of the batch; None: the identity
      mask        [H,W], [1,H,W], or [B,1,H,W] for one mask per image; None: ones
    With exposure=None and mask=None the three values and the gradient are r3dgs_loss.l1_dssim's bit for bit."""
    what = "exposed_l1_dssim"
    _check_image(what, image)
    e_per_image = _check_exposure(what, exposure, image) if exposure is not None else False
    m_per_image = _check_mask(what, mask, image) if mask is not None else False
    _check_pair(what, image, gt)
    _check_devices(what, image, exposure=exposure, mask=mask)
    return _ExposedL1DSSIM.apply(image, gt, exposure, mask, (e_per_image, m_per_image, bool(mask_target)), float(lambda_dssim))


@torch.no_grad()
def apply_exposure(image, exposure, clamp=False):
    """image E[:, :3] + E[:, 3] per pixel, clamped to [0, 1] with clamp=True: the exposed render for evaluation and saving
    (train_test_exp).  image [3,H,W] or [B,3,H,W]; exposure [3,4] or [B,3,4].  One launch; no gradient."""
    what = "apply_exposure"
    _check_image(what, image)
    if image.dtype != torch.float32:
        raise TypeError(f"{what}: image is {image.dtype}; float32 only")
    per_image = _check_exposure(what, exposure, image)
    _check_devices(what, image, prediction=image, exposure=exposure)
    B, _, H, W = _bchw(image)
    return _C.exposure_apply(image.contiguous(), exposure.detach().contiguous(), per_image, bool(clamp), B, H, W).view(image.shape)


class ExposureTable(torch.nn.Module):
    """One learnable 3 x 4 exposure per training image, initialised to the identity eye(3, 4) (the official `_exposure`
    parameter).  table[idx] is the [3,4] view to hand to exposed_l1_dssim / apply_exposure (a tensor of indices gives [n,3,4]);
    table.parameters() goes to torch.optim.Adam or r3dgs_optim.Adam; state_dict() round-trips."""

    def __init__(self, n_images):
        super().__init__()
        if int(n_images) < 1:
            raise ValueError(f"ExposureTable: n_images = {n_images}")
        self.exposure = torch.nn.Parameter(torch.eye(3, 4).repeat(int(n_images), 1, 1))

    def __len__(self):
        return self.exposure.shape[0]

    def __getitem__(self, idx):
        return self.exposure[idx]
