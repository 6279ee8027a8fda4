"""`r3dgs_train_stats` -- the visibility-masked bookkeeping of a training iteration on the MI355X, in HIP
(csrc/train_stats.hip, include/r3dgs_trainstats.h), without a host wait.

    from r3dgs_train_stats import visible_means, add_densification_stats

    vm = visible_means(radii, opacity=gaussians._opacity, features_rest=gaussians._features_rest)
    Lalpha_regul = vm.alpha_mean                       # train.py:105-106  get_opacity[visibility_filter].abs().mean()
    sh_sparsity_loss = lambda_sh * vm.sh_abs_mean      # train.py:113      _features_rest.detach()[visibility_filter].abs().mean()
    ...loss.backward()...
    add_densification_stats(gaussians, viewspace_point_tensor, radii)     # train.py:134, gaussian_model.py:693-695

The reference writes these lines with boolean-mask indexing; every `x[mask]` runs `nonzero`, which blocks the host until the
stream has drained.  Here `radii > 0` is applied inside the kernels: the count of visible Gaussians stays on the device and
nothing is gathered.  `opacity` is the RAW parameter (`_opacity`); the sigmoid is applied in the kernel.  Host tensors are
refused (there is no CPU path); the calls can be captured in torch.cuda.graph; the results are bit-identical from run to run.
"""
from typing import NamedTuple, Optional

import torch

from diff_gaussian_rasterization import _C

__all__ = ["VisibleMeans", "visible_means", "densification_stats", "add_densification_stats"]


class VisibleMeans(NamedTuple):
    visibility_filter: torch.Tensor          # bool [P]: radii > 0
    n_visible: torch.Tensor                  # int32, 0-d, on the device
    alpha_mean: Optional[torch.Tensor]       # fp32, 0-d: mean sigmoid(opacity) over the visible Gaussians (None: no opacity)
    sh_abs_mean: Optional[torch.Tensor]      # fp32, 0-d: mean |features_rest| over their rows (None: no features_rest)


def _tensor(what, name, t, dtype, shape_ok, shape_text):
    """dtype and shape first, so that a wrong tensor is named for what is wrong with it wherever it lives"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {name} is {t.dtype}, expected {dtype}")
    if not shape_ok(t):
        raise ValueError(f"{what}: {name} must be {shape_text}, got {tuple(t.shape)}")


def _on_one_gpu(what, **tensors):
    dev = None
    for name, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} is a host tensor; the training statistics need device tensors (no CPU path)")
        if dev is not None and t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, expected {dev}")
        dev = t.device


class _AlphaMean(torch.autograd.Function):
    """alpha_mean with its backward; the other outputs ride along without a gradient."""

    @staticmethod
    def forward(ctx, opacity, radii, features_rest):
        vis, n, alpha, sh = _C.visible_means(radii, opacity, features_rest)
        ctx.save_for_backward(radii, opacity, n)
        outs = (vis, n) if sh is None else (vis, n, sh)
        ctx.mark_non_differentiable(*outs)
        return (alpha,) + outs

    @staticmethod
    def backward(ctx, g_alpha, *_):
        radii, opacity, n = ctx.saved_tensors
        grad = torch.zeros_like(opacity)
        # the upstream scalar goes to the kernel as a tensor: nothing is read back
        _C.alpha_regul_backward(radii, opacity, g_alpha.to(torch.float32).contiguous(), n, grad)
        return grad, None, None


def visible_means(radii, opacity=None, features_rest=None):
    """-> VisibleMeans.  radii: int32 [P] as the rasterizer returns it; opacity: the raw fp32 [P,1] (or [P]) parameter;
    features_rest: fp32 [P, M-1, 3].  alpha_mean is an autograd scalar when opacity requires grad (its backward is one
    elementwise launch); sh_abs_mean carries no gradient, as the reference detaches it.  Means of nothing are NaN, as
    torch's: no visible Gaussian, or M == 1 for sh_abs_mean."""
    what = "visible_means"
    _tensor(what, "radii", radii, torch.int32, lambda t: t.dim() == 1, "[P]")
    P = radii.numel()
    tensors = {"radii": radii}
    if opacity is not None:
        _tensor(what, "opacity", opacity, torch.float32, lambda t: t.numel() == P and t.dim() in (1, 2),
                f"[P] or [P,1] with P = {P}")
        tensors["opacity"] = opacity
    if features_rest is not None:
        _tensor(what, "features_rest", features_rest, torch.float32,
                lambda t: t.dim() == 3 and t.size(0) == P and t.size(2) == 3, f"[P, M-1, 3] with P = {P}")
        tensors["features_rest"] = features_rest
    _on_one_gpu(what, **tensors)
    radii = radii.contiguous()
    if opacity is not None:
        opacity = opacity.contiguous()
    if features_rest is not None:
        features_rest = features_rest.detach().contiguous()
    if opacity is None:
        vis, n, _, sh = _C.visible_means(radii, None, features_rest)
        return VisibleMeans(vis, n, None, sh)
    out = _AlphaMean.apply(opacity, radii, features_rest)
    return VisibleMeans(out[1], out[2], out[0], out[3] if features_rest is not None else None)


def densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """In place, one launch (train.py:134, scene/gaussian_model.py:693-695), with vis = radii > 0:
        xyz_gradient_accum += vis ? ||viewspace_grad[:, :2]|| : 0;  denom += vis;  max_radii2D = vis ? max(., radii) : .
    viewspace_grad: fp32 [P,3]; xyz_gradient_accum, denom: fp32 [P,1]; max_radii2D: fp32 [P].  The accumulators are updated
    where they are: one of the wrong dtype, shape or layout is refused, never copied."""
    what = "densification_stats"
    _tensor(what, "radii", radii, torch.int32, lambda t: t.dim() == 1, "[P]")
    P = radii.numel()
    _tensor(what, "viewspace_grad", viewspace_grad, torch.float32, lambda t: tuple(t.shape) == (P, 3), f"[P,3] with P = {P}")
    accumulators = {"xyz_gradient_accum": (xyz_gradient_accum, (P, 1)), "denom": (denom, (P, 1)), "max_radii2D": (max_radii2D, (P,))}
    for name, (t, shape) in accumulators.items():
        _tensor(what, name, t, torch.float32, lambda x: tuple(x.shape) == shape, str(list(shape)))
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous; it is updated in place and is not copied")
        if t.requires_grad:
            raise RuntimeError(f"{what}: {name} requires grad; it is updated in place")
    _on_one_gpu(what, radii=radii, viewspace_grad=viewspace_grad, **{k: v[0] for k, v in accumulators.items()})
    radii = radii.contiguous()
    _C.densification_stats(viewspace_grad.detach().contiguous(), radii, xyz_gradient_accum, denom, max_radii2D)


def add_densification_stats(pc, viewspace_point_tensor, radii):
    """train.py:134 + GaussianModel.add_densification_stats (scene/gaussian_model.py:693-695) for anything with the reference
    model's three attributes: pc.xyz_gradient_accum, pc.denom and pc.max_radii2D are updated in place.
    viewspace_point_tensor: the means2D dummy after backward() (its .grad is read), or the [P,3] gradient itself."""
    grad = viewspace_point_tensor
    if isinstance(grad, torch.Tensor) and grad.requires_grad:
        if grad.grad is None:
            raise RuntimeError("add_densification_stats: viewspace_point_tensor has no .grad yet (call backward() first)")
        grad = grad.grad
    densification_stats(grad, radii, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)


def add_densification_stats_absgrad(pc, viewspace_point_tensor, radii):
    """add_densification_stats with the AbsGS signal: the norm accumulated is that of viewspace_point_tensor.absgrad -- what
    render(..., absgrad=True) leaves there after backward() -- through the same kernel (the tensor is [P,3] like .grad)."""
    grad = getattr(viewspace_point_tensor, "absgrad", None)
    if not isinstance(grad, torch.Tensor):
        raise RuntimeError("add_densification_stats_absgrad: viewspace_point_tensor has no .absgrad (render with absgrad=True "
                           "and call backward() first)")
    densification_stats(grad, radii, pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)
