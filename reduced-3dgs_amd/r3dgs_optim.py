"""`r3dgs_optim` -- the optimizer of scene/gaussian_model.py:217 on the MI355X: one fused HIP launch per step for every
parameter group (csrc/optim.hip, include/r3dgs_optim.h) instead of torch's ~8 elementwise passes per group.

    self.optimizer = r3dgs_optim.Adam(l, lr=0.0, eps=1e-15)     # instead of torch.optim.Adam(l, lr=0.0, eps=1e-15)

Same constructor defaults, parameter groups, state keys and lazy state initialisation as torch.optim.Adam, and the same
results bit for bit as its default (foreach) step for fp32 device tensors (csrc/adam_math.h states the roundings).  The
state is re-read on every step, so the reference's update_learning_rate, replace_tensor_to_optimizer, _prune_optimizer,
cat_tensors_to_optimizer, capture() / restore() and zero_grad(set_to_none=True) work unchanged, and checkpoints load in
both directions between this class and torch.optim.Adam.

Refused, each with a message: amsgrad, maximize, weight_decay != 0, differentiable, the foreach / fused arguments, tensors
that are not float32, host, sparse, complex or non-contiguous tensors, a parameter whose state differs from it in shape, and
a step() during stream capture unless capturable=True.  With capturable=True the step count lives on the device, the kernel
bumps it and computes the bias corrections from it, and lr may be a 0-d float32 device tensor read at replay; that
arithmetic is close to torch's capturable step but not bit-identical to it.

The visibility-gated step (opt-in): `step(radii=radii)` with the rasterizer's radii of the view just rendered, an int32,
contiguous, 1-d device tensor [P], updates only the Gaussians that view rendered.  Every parameter with a gradient must be
[P, ...].  Row i is visible iff radii[i] > 0 (zero and negative are both invisible).

  * a visible row takes exactly the dense step's arithmetic (the same csrc/adam_math.h function) with this step's scalars;
  * an invisible row keeps the bits of its parameter, exp_avg and exp_avg_sq, and its gradient is not looked at: NaN or
    Inf there reaches nothing;
  * state['step'] is one count per tensor, bumped once per step() whatever was visible, and the bias corrections come
    from it -- torch.optim.SparseAdam's row semantics; state keys, lazy initialisation and checkpoints are unchanged;
  * with every row visible the result equals step() without radii bit for bit, plain and capturable; with capturable=True
    radii is read at replay, so a captured graph follows new contents of the same buffer.

This is NOT the dense step's arithmetic where a view culls: under torch.optim.Adam a culled row (g = 0) still decays exp_avg
and exp_avg_sq and still moves the parameter on its momentum; here it does neither.  Training results therefore differ from
the reference's default optimizer (official 3DGS offers the same trade as --optimizer_type sparse_adam).  No 30k-iteration
PSNR comparison exists for either optimizer with this rasterizer.  step() without radii stays the default and is unchanged.
"""
import torch

from diff_gaussian_rasterization import _C

__all__ = ["Adam"]

_REFUSED = (("amsgrad", False), ("maximize", False), ("differentiable", False), ("foreach", None), ("fused", None),
            ("decoupled_weight_decay", False))


def _check_group(group):
    for key, allowed in _REFUSED:
        if group.get(key, allowed) != allowed:
            raise ValueError(f"r3dgs_optim.Adam: {key}={group[key]!r} is not supported (the fused step implements "
                             f"torch.optim.Adam's default step; {key} must be {allowed!r})")
    if group.get("weight_decay", 0) != 0:
        raise ValueError(f"r3dgs_optim.Adam: weight_decay={group['weight_decay']!r} is not supported (must be 0)")
    beta1, beta2 = group["betas"]
    if isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor) or isinstance(group["eps"], torch.Tensor):
        raise ValueError("r3dgs_optim.Adam: betas and eps must be Python floats")
    if isinstance(group["lr"], torch.Tensor) and not group["capturable"]:
        raise ValueError("r3dgs_optim.Adam: a Tensor lr needs capturable=True")


def _check_tensor(what, t, p):
    if t.is_sparse:
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is sparse; the fused step takes dense tensors only")
    if t.is_complex():
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is complex ({t.dtype}); the fused step takes float32 only")
    if t.dtype != torch.float32:
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is {t.dtype}; the fused step takes float32 only")
    if not t.is_cuda:
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is a host tensor; the fused step needs device tensors (no CPU path)")
    if t.device != p.device:
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is on {t.device}, its parameter on {p.device}")
    if t.shape != p.shape:
        raise RuntimeError(f"r3dgs_optim.Adam: {what} has shape {tuple(t.shape)}, its parameter {tuple(p.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"r3dgs_optim.Adam: {what} is not contiguous; the fused step takes contiguous tensors only")


def _check_radii(radii, param_groups):
    """The gated step's own refusals, each naming its offender, before any state is made or any count bumped."""
    if not isinstance(radii, torch.Tensor):
        raise TypeError(f"r3dgs_optim.Adam: radii is a {type(radii).__name__}; the gated step takes the rasterizer's int32 "
                        "tensor")
    if radii.dtype != torch.int32:
        raise RuntimeError(f"r3dgs_optim.Adam: radii is {radii.dtype}; the gated step takes the rasterizer's int32 radii")
    if radii.dim() != 1:
        raise RuntimeError(f"r3dgs_optim.Adam: radii has shape {tuple(radii.shape)}; the gated step takes a 1-d tensor [P]")
    if not radii.is_contiguous():
        raise RuntimeError("r3dgs_optim.Adam: radii is not contiguous; the gated step takes a contiguous tensor only")
    for gi, group in enumerate(param_groups):
        for pi, p in enumerate(group["params"]):
            if p.grad is not None and (p.dim() < 1 or p.shape[0] != radii.numel()):
                name = group.get("name")
                what = f"parameter {pi} of group {gi}" + (f" ({name!r})" if name is not None else "")
                raise RuntimeError(f"r3dgs_optim.Adam: {what} has shape {tuple(p.shape)}, but radii has {radii.numel()} "
                                   "rows; the gated step needs every parameter as [P, ...] with P == radii.numel()")
    if not radii.is_cuda:
        raise RuntimeError("r3dgs_optim.Adam: radii is a host tensor; the gated step needs a device tensor (no CPU path)")
    for group in param_groups:
        for p in group["params"]:
            if p.grad is not None and p.device != radii.device:
                raise RuntimeError(f"r3dgs_optim.Adam: radii is on {radii.device}, a parameter on {p.device}")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's interface and default step, fused into one HIP launch per step (see the module docstring)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("r3dgs_optim.Adam: a Tensor lr must have one element")
        elif not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=False)
        _check_group(defaults)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for key, default in _REFUSED + (("capturable", False),):
                group.setdefault(key, default)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        _check_group(self.param_groups[-1])

    @torch.no_grad()
    def step(self, closure=None, *, radii=None):
        """One step; with radii (the rasterizer's int32 [P] of the view just rendered) only the rows with radii > 0 are
        updated and the others keep their bits (see the module docstring)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if radii is not None:
            _check_radii(radii, self.param_groups)
        plain, capt = {}, {}   # device -> the launch's lists
        bumps = []             # (state['step'], its bumped value): stored once every tensor has passed its checks
        for group in self.param_groups:
            _check_group(group)
            capturable = group["capturable"]
            if capturing and not capturable:
                raise RuntimeError("r3dgs_optim.Adam: step() during stream capture needs capturable=True (the host scalars "
                                   "of the default step would be baked into the graph)")
            beta1, beta2 = group["betas"]
            eps, lr = group["eps"], group["lr"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check_tensor("a gradient", p.grad, p)
                _check_tensor("a parameter", p, p)
                state = self.state[p]
                if len(state) == 0:   # torch's lazy initialisation: the same keys, dtypes and devices
                    state["step"] = (torch.zeros((), dtype=torch.float32, device=p.device) if capturable
                                     else torch.tensor(0.0, dtype=torch.float32))
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v, step_t = state["exp_avg"], state["exp_avg_sq"], state["step"]
                _check_tensor("exp_avg", m, p)
                _check_tensor("exp_avg_sq", v, p)
                if capturable:
                    if step_t.device != p.device or step_t.dtype != torch.float32 or step_t.numel() != 1:
                        raise RuntimeError("r3dgs_optim.Adam: capturable=True needs state['step'] as a float32 tensor on the "
                                           "parameter's device")
                    lr_t = _EMPTY
                    if isinstance(lr, torch.Tensor):
                        if lr.is_cuda:
                            if lr.device != p.device or lr.dtype != torch.float32 or lr.numel() != 1:
                                raise RuntimeError("r3dgs_optim.Adam: a device lr must be a one-element float32 tensor on "
                                                   "the parameters' device")
                            lr_t = lr
                        lr_value = 0.0 if lr.is_cuda else float(lr)
                    else:
                        lr_value = float(lr)
                    d = capt.setdefault(p.device, ([], [], [], [], [], [], []))
                    for lst, t in zip(d, (p, p.grad, m, v, step_t, lr_t)):
                        lst.append(t)
                    d[6].extend((lr_value, float(beta1), float(beta2), float(eps)))
                else:
                    if step_t.is_cuda:
                        raise RuntimeError("r3dgs_optim.Adam: state['step'] is on the device but capturable=False (torch "
                                           "keeps it on the host there)")
                    bumped = step_t + 1   # the count after this step's bump: torch adds 1.0 to the fp32 CPU tensor
                    bumps.append((step_t, bumped))
                    step = bumped.item()
                    # torch/optim/adam.py's host scalars, in Python doubles; _C rounds each to fp32 once
                    bias_correction1 = 1 - beta1 ** step
                    bias_correction2 = 1 - beta2 ** step
                    step_size = (lr / bias_correction1) * -1
                    bias_correction2_sqrt = bias_correction2 ** 0.5
                    d = plain.setdefault(p.device, ([], [], [], [], []))
                    for lst, t in zip(d, (p, p.grad, m, v)):
                        lst.append(t)
                    d[4].extend((1 - beta1, beta2, 1 - beta2, bias_correction2_sqrt, eps, step_size))
        for step_t, bumped in bumps:
            step_t.copy_(bumped)
        for params, grads, ms, vs, scalars in plain.values():
            if radii is None:
                _C.adam_step(params, grads, ms, vs, scalars)
            else:
                _C.adam_step_visible(params, grads, ms, vs, scalars, radii)
        for params, grads, ms, vs, steps, lrs, scalars in capt.values():
            if radii is None:
                _C.adam_step_capturable(params, grads, ms, vs, steps, lrs, scalars)
            else:
                _C.adam_step_capturable_visible(params, grads, ms, vs, steps, lrs, scalars, radii)
        return loss


_EMPTY = torch.Tensor([])
