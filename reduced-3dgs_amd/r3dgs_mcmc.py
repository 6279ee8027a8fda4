"""`r3dgs_mcmc` -- the fixed-budget densification strategy of 3DGS-MCMC (Kheradmand et al., 2024) on the MI355X in HIP
(csrc/mcmc.hip, csrc/mcmc_math.h, include/r3dgs_mcmc.h).  It is NOT the reference's densify_and_prune (r3dgs_densify): the
Gaussian count is capped, dead Gaussians are relocated onto live ones instead of pruned, the model grows by 5 % per refinement
until it reaches the cap, and a small opacity-gated noise term shaped by each Gaussian's covariance moves the positions every
iteration.

    from r3dgs_mcmc import MCMCStrategy, regularisation

    strategy = MCMCStrategy(cap_max=1_000_000)
    loss = loss + regularisation(gaussians)                       # before backward()
    strategy.step_post_backward(gaussians, iteration, xyz_lr)     # after optimizer.step()

`pc` is anything shaped like the reference's GaussianModel, as for r3dgs_densify: `_xyz`, `_features_dc`, `_features_rest`,
`_opacity`, `_scaling`, `_rotation`, `_degrees` and `optimizer`, whose groups are named "xyz", "f_dc", "f_rest", "opacity",
"scaling", "rotation" with one parameter each (torch.optim.Adam or r3dgs_optim.Adam, plain or capturable; a group without state
yet has only its parameter moved).  `xyz_gradient_accum`, `denom` and `max_radii2D` are reset by add_new where the model has them.

No call waits on the host: the number of dead rows is counted and used on the device, and the new size of add_new is a
function of P and the cap alone.  Statistics come back as device tensors; nothing is read back unless the caller does it.
inject_noise and relocate change no size and are capturable in a graph (pass `noise` / `uniforms` explicitly then).

Randomness is the caller's, as in r3dgs_densify: `noise` is standard-normal float32 [P,3] (torch.randn with `generator` when
None), `uniforms` float32 in [0,1) (torch.rand with `generator` when None): P entries for relocate, n_new for add_new.

Host tensors are refused (no CPU path), as are non-contiguous tensors, wrong dtypes and tensors whose first dimension is not P.
"""
import torch

import r3dgs_model_state as ms
from diff_gaussian_rasterization import _C

__all__ = ["inject_noise", "relocate", "add_new", "regularisation", "n_new_rows", "MCMCStrategy"]

_lib = _C._lib   # the r3dgs_mcmc_* prototypes are rows of the required group of _C's ABI table
_Tensor = _C._McmcTensor

RELOCATE, GROW = 0, 1                          # R3DGS_MCMC_RELOCATE / _GROW
COPY, MOMENT, OPACITY, SCALING = 0, 1, 2, 3    # R3DGS_MCMC_*
MAX_TENSORS, TOTALS, MAX_RATIO = 32, 8, 51
GROW_MIN_OPACITY = 0.005   # the lower clamp of a grown source's new opacity: the strategy's default min_opacity

_KIND = {"opacity": OPACITY, "scaling": SCALING}
_f32 = ms.f32


def _extra(what, name, t, shape, shape_text):
    ms.check_extra(what, name, t, torch.float32, shape, shape_text)


def _stats(totals, sampled, slots, ratio):
    """The plan's outputs, all on the device: the counters are 0-d views of `totals`."""
    return {"n_dead": totals[0], "n_draws": totals[1], "n_sources": totals[2], "n_clamped": totals[3], "noop": totals[4],
            "totals": totals, "sampled": sampled, "slots": slots, "ratio": ratio}


def inject_noise(pc, scale, noise=None, generator=None):
    """pc._xyz += scale * gate(opacity) * (covariance @ noise row), in place, in one launch; scale = noise_lr * the current
    learning rate of xyz.  A zero noise row leaves its xyz row bit for bit.  Capturable in a graph when `noise` is given."""
    what = "inject_noise"
    P = ms.model_size(what, pc)
    if noise is not None:
        _extra(what, "noise", noise, (P, 3), f"(P, 3) with P = {P}")
    tensors = (("pc._xyz", pc._xyz, (3,)), ("pc._opacity", pc._opacity, (1,)), ("pc._scaling", pc._scaling, (3,)),
               ("pc._rotation", pc._rotation, (4,)))
    for name, t, width in tensors:
        ms.check(what, name, t, torch.float32, P)
        if tuple(t.shape[1:]) != width:
            raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {(P,) + width}")
    dev = pc._xyz.device
    ms.check_devices(what, [t for _, t, _ in tensors], dev)
    if noise is not None:
        ms.check_extra_device(what, "noise", noise, dev)
    if P == 0:
        return
    with torch.no_grad(), _C._on_device(dev):
        if noise is None:
            noise = torch.randn((P, 3), generator=generator, device=dev, dtype=torch.float32)
        _C._check(_lib.r3dgs_mcmc_noise(P, pc._xyz.data_ptr(), pc._opacity.data_ptr(), pc._scaling.data_ptr(),
                                        pc._rotation.data_ptr(), noise.data_ptr(), _f32(scale), _C._stream()), what)


def relocate(pc, min_opacity=0.005, uniforms=None, generator=None, zero_relocated=False):
    """Every dead Gaussian (sigmoid(opacity) <= min_opacity) becomes a copy of a live one drawn with probability proportional
    to its opacity; the drawn sources take the opacity and scales that keep the rendered result (include/r3dgs_mcmc.h), and
    their Adam moments are zeroed.  The relocated rows keep their own moments unless zero_relocated.  In place: no tensor
    object is replaced, state['step'] is untouched.  -> a dict of device tensors (n_dead, n_draws, n_sources, n_clamped, noop,
    totals, sampled, slots, ratio).  Capturable in a graph when `uniforms` is given."""
    what = "relocate"
    P = ms.model_size(what, pc)
    if uniforms is not None:
        _extra(what, "uniforms", uniforms, (P,), f"(P,) with P = {P}")
    P, dev, entries = ms.collect(what, pc, _KIND, MOMENT)   # the accumulators are not looked at
    if uniforms is not None:
        ms.check_extra_device(what, "uniforms", uniforms, dev)
    with torch.no_grad(), _C._on_device(dev):
        stream = _C._stream()
        totals = torch.empty((TOTALS,), dtype=torch.int32, device=dev)
        sampled = torch.empty((P,), dtype=torch.int32, device=dev)
        slots = torch.empty((P,), dtype=torch.int32, device=dev)
        ratio = torch.empty((P,), dtype=torch.int32, device=dev)
        if uniforms is None and P > 0:
            uniforms = torch.rand((P,), generator=generator, device=dev, dtype=torch.float32)
        ws = torch.empty((int(_lib.r3dgs_mcmc_workspace_bytes(P, P)),), dtype=torch.uint8, device=dev) if P > 0 else None
        _C._check(_lib.r3dgs_mcmc_plan(P, pc._opacity.data_ptr() if P else None, _f32(min_opacity), RELOCATE, P,
                                       uniforms.data_ptr() if P else None, sampled.data_ptr() if P else None,
                                       slots.data_ptr() if P else None, ratio.data_ptr() if P else None, totals.data_ptr(),
                                       ws.data_ptr() if P else None, stream), what)
        if P > 0:
            table = ms.fill_table(_Tensor, entries, [t for _, t, _ in entries], P)
            _C._check(_lib.r3dgs_mcmc_move(P, RELOCATE, 0, 1 if zero_relocated else 0, _f32(min_opacity), len(entries), table,
                                           pc._opacity.data_ptr(), pc._scaling.data_ptr(), sampled.data_ptr(), slots.data_ptr(),
                                           ratio.data_ptr(), totals.data_ptr(), ws.data_ptr(), stream), what)
    return _stats(totals, sampled, slots, ratio)


def n_new_rows(P, cap_max, growth=1.05):
    """Rows add_new appends to a model of P Gaussians: max(0, min(cap_max, int(growth * P)) - P)."""
    return max(0, min(int(cap_max), int(growth * P)) - P)


def add_new(pc, cap_max, growth=1.05, uniforms=None, generator=None):
    """Grows the model to min(cap_max, int(growth * P)) Gaussians: each new row is a copy of a source drawn with probability
    proportional to its opacity, after the drawn sources took the opacity and scales that keep the rendered result.  Moments:
    old rows keep theirs, new rows get zeros; xyz_gradient_accum, denom and max_radii2D become zeros of the new size where
    the model has them; the optimizer state is re-keyed as r3dgs_densify does it.  With nothing to add nothing changes and
    no tensor object is replaced.  -> a dict of device tensors as relocate's (slots is None), plus "n_new" (a Python int)."""
    what = "add_new"
    P = ms.model_size(what, pc)
    n_new = n_new_rows(P, cap_max, growth)
    if uniforms is not None:
        _extra(what, "uniforms", uniforms, (n_new,), f"(n_new,) with n_new = {n_new}")
    P, dev, entries = ms.collect(what, pc, _KIND, MOMENT)   # the accumulators are not looked at
    if uniforms is not None:
        ms.check_extra_device(what, "uniforms", uniforms, dev)
    with torch.no_grad(), _C._on_device(dev):
        stream = _C._stream()
        totals = torch.empty((TOTALS,), dtype=torch.int32, device=dev)
        sampled = torch.empty((n_new,), dtype=torch.int32, device=dev)
        ratio = torch.empty((P,), dtype=torch.int32, device=dev)
        if n_new == 0:   # nothing changes; the statistics say so
            totals.zero_()
            totals[4] = 2
            ratio.fill_(1)
            return dict(_stats(totals, sampled, None, ratio), n_new=0)
        if uniforms is None:
            uniforms = torch.rand((n_new,), generator=generator, device=dev, dtype=torch.float32)
        ws = torch.empty((int(_lib.r3dgs_mcmc_workspace_bytes(P, n_new)),), dtype=torch.uint8, device=dev)
        _C._check(_lib.r3dgs_mcmc_plan(P, pc._opacity.data_ptr(), 0.0, GROW, n_new, uniforms.data_ptr(), sampled.data_ptr(), None,
                                       ratio.data_ptr(), totals.data_ptr(), ws.data_ptr(), stream), what)
        rows = P + n_new
        new = ms.new_rows(entries, rows, dev)
        table = ms.fill_table(_Tensor, entries, new, P)
        _C._check(_lib.r3dgs_mcmc_move(P, GROW, n_new, 0, _f32(GROW_MIN_OPACITY), len(entries), table, pc._opacity.data_ptr(),
                                       pc._scaling.data_ptr(), sampled.data_ptr(), None, ratio.data_ptr(), totals.data_ptr(),
                                       ws.data_ptr(), stream), what)
        ms.hand_over(pc, entries, new)
        for name in ms.ACCUMULATORS:
            old = getattr(pc, name, None)
            if isinstance(old, torch.Tensor):
                setattr(pc, name, torch.zeros((rows,) + tuple(old.shape[1:]), dtype=old.dtype, device=dev))
    return dict(_stats(totals, sampled, None, ratio), n_new=n_new)


def regularisation(pc, opacity_reg=0.01, scale_reg=0.01):
    """The two mean terms the method adds to the loss: opacity_reg * mean(sigmoid(opacity)) + scale_reg * mean(exp(scaling)).
    Plain torch, differentiable."""
    return opacity_reg * torch.sigmoid(pc._opacity).abs().mean() + scale_reg * torch.exp(pc._scaling).abs().mean()


class MCMCStrategy:
    """The schedule of 3DGS-MCMC: on a refinement iteration (refine_start < iteration < refine_stop, every refine_every)
    relocate and then grow; on every iteration inject noise of scale noise_lr * xyz_lr.  Call it after optimizer.step()."""

    def __init__(self, cap_max, noise_lr=5e5, refine_start=500, refine_stop=25000, refine_every=100, min_opacity=0.005,
                 generator=None):
        self.cap_max, self.noise_lr = int(cap_max), float(noise_lr)
        self.refine_start, self.refine_stop, self.refine_every = refine_start, refine_stop, refine_every
        self.min_opacity, self.generator = min_opacity, generator

    def is_refinement(self, iteration):
        return self.refine_start < iteration < self.refine_stop and iteration % self.refine_every == 0

    def step_post_backward(self, pc, iteration, xyz_lr):
        """-> {"relocate": ..., "add_new": ...} (the two calls' device statistics) on a refinement iteration, else None."""
        stats = None
        if self.is_refinement(iteration):
            stats = {"relocate": relocate(pc, self.min_opacity, generator=self.generator),
                     "add_new": add_new(pc, self.cap_max, generator=self.generator)}
        inject_noise(pc, self.noise_lr * xyz_lr, generator=self.generator)
        return stats
