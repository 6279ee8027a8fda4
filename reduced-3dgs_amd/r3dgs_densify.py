"""`r3dgs_densify` -- densification on the MI355X in HIP (csrc/densify.hip, include/r3dgs_densify.h): clone, split and prune
of the Gaussians, of both Adam moments of every parameter, of `_degrees` and of the accumulators as ONE read and one write of
the state, with one host wait.

    from r3dgs_densify import densify_and_prune, prune, prune_points

    densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size, stats_dict)   # train.py:139
    prune(gaussians, min_opacity, extent, max_screen_size, stats_dict)                         # train.py:144, :165
    prune_points(gaussians, mask)                                                              # gaussian_model.py:548

`pc` is anything shaped like the reference's GaussianModel: `_xyz`, `_features_dc`, `_features_rest`, `_opacity`, `_scaling`,
`_rotation`, `_degrees`, `xyz_gradient_accum`, `denom`, `max_radii2D`, `percent_dense` and `optimizer`, whose groups are
named "xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation" with one parameter each.  The reference runs these calls as
some 80 torch launches that copy every tensor up to four times (cat, cat, mask-index, mask-index) and wait on the host about
a dozen times (scene/gaussian_model.py:502-691).

Semantics: the reference's, restated line by line in tests/densify_ref.py, quirks included:
  * the result is four stable segments in source order: surviving originals, surviving clones, surviving first children,
    surviving second children; exp_avg / exp_avg_sq rows follow their parameter row in the first and are zero in the others,
    state['step'] is untouched, and the optimizer's state is re-keyed as _prune_optimizer / cat_tensors_to_optimizer do it
    (the old key deleted, the SAME state dict under the new parameter, group["params"][0] replaced);
  * inside densify_and_prune the screen-size term of the prune mask never acts: densification_postfix has zeroed max_radii2D
    before prune() looks at it.  It acts when prune() is called on its own;
  * the children's world-size term looks at exp(log(scale / 1.6)), the activation of the stored child scale;
  * max_grad <= 0 is refused: the reference takes the split decision after the clones were appended with a zero gradient,
    so it would split the clones;
  * a group without optimizer state (before the first step) gets its parameter moved and nothing else; with store_grads
    the `.grad` rows move like the moments, but only for a group that has state (as gaussian_model.py:511-515);
  * after a densify, xyz_gradient_accum, denom, max_radii2D and density_gradient_accum are zeros of the new size; after
    prune() and prune_points() the first three are compacted and density_gradient_accum is left alone, as in the reference.

Noise: `noise` is standard-normal float32 [2, P, 3] indexed by (child, SOURCE Gaussian); only the rows of split parents are
read.  With noise=None it is drawn as torch.randn((2, P, 3), generator=generator) on the device.  This is the reference's
distribution (torch.normal(mean=0, std=s) is randn * s), not its random stream: the reference draws [2 n_split, 3].

The calls read eight integers back once (the new sizes: they have to size the new tensors), so they are NOT capturable in a
graph; nothing else waits.  No empty_cache().  P == 0 before or after is valid.  Host tensors are refused (no CPU path), as
are non-contiguous tensors, wrong dtypes and tensors whose first dimension is not P.  n_points_cloned, n_points_split and
n_points_pruned are stored as Python ints.
"""
import torch

import r3dgs_model_state as ms
from diff_gaussian_rasterization import _C

__all__ = ["densify_and_prune", "prune", "prune_points"]

_lib = _C._lib   # the r3dgs_densify_* / r3dgs_prune_plan prototypes are rows of _C's ABI table
_C._need("densify", ImportError)

COPY, ZERO_NEW, XYZ, SCALING = 0, 1, 2, 3     # R3DGS_DENSIFY_*
MAX_TENSORS, TOTALS = 32, 8

_Tensor = _C._DensifyTensor   # r3dgs_densify_tensor: the struct sits next to the table that declares the pointer to it
_GROUPS = ms.GROUPS
_CHILD_KIND = {"xyz": XYZ, "scaling": SCALING}
_f32 = ms.f32


def _run(what, pc, entries, P, dev, plan, noise, zero_accumulators):
    """plan (enqueue) -> the one read-back -> new tensors -> move (enqueue) -> hand the new tensors to the model and the
    optimizer.  -> the eight totals."""
    with torch.no_grad(), _C._on_device(dev):
        stream = _C._stream()
        if P > 0:
            ws = torch.empty((int(_lib.r3dgs_densify_workspace_bytes(P)),), dtype=torch.uint8, device=dev)
            totals_dev = torch.empty((TOTALS,), dtype=torch.int32, device=dev)
            _C._check(plan(ws.data_ptr(), totals_dev.data_ptr(), stream), what)
            totals = totals_dev.tolist()          # the only host wait of the call: the new sizes
        else:
            ws, totals = None, [0] * TOTALS
        nA, nB, nC, _, _, _, _, rows = totals
        new = ms.new_rows(entries, rows, dev)
        if rows > 0:
            table = ms.fill_table(_Tensor, entries, new, P)
            _C._check(_lib.r3dgs_densify_move(P, nA, nB, nC, len(entries), table, pc._xyz.data_ptr(), pc._scaling.data_ptr(),
                                              pc._rotation.data_ptr(), noise.data_ptr() if noise is not None else None,
                                              ws.data_ptr(), stream), what)
        ms.hand_over(pc, entries, new)
        if zero_accumulators:   # densification_postfix, gaussian_model.py:617-620
            pc.xyz_gradient_accum = torch.zeros((rows, 1), device=dev)
            pc.density_gradient_accum = torch.zeros((rows, 1), device=dev)
            pc.denom = torch.zeros((rows, 1), device=dev)
            pc.max_radii2D = torch.zeros((rows,), device=dev)
    return totals


def densify_and_prune(pc, max_grad, min_opacity, extent, max_screen_size, densification_statistics_dict, store_grads=False,
                      noise=None, generator=None):
    """GaussianModel.densify_and_prune (scene/gaussian_model.py:670-682) in three launches and one host wait; see the module
    docstring for the semantics, the kept quirks and the noise convention.  Not capturable in a graph: the sizes change."""
    what = "densify_and_prune"
    if not max_grad > 0:
        raise ValueError(f"{what}: max_grad = {max_grad!r} must be > 0 (the reference takes the split decision after the clones "
                         "were appended with a zero gradient: max_grad <= 0 would split the clones)")
    if noise is not None:
        P = ms.model_size(what, pc)
        ms.check_extra(what, "noise", noise, torch.float32, (2, P, 3), f"(2, P, 3) with P = {P}")
    P, dev, entries = ms.collect(what, pc, _CHILD_KIND, ZERO_NEW, store_grads, accumulators=False)
    if noise is None:
        noise = torch.randn((2, P, 3), generator=generator, device=dev, dtype=torch.float32)
    else:
        ms.check_extra_device(what, "noise", noise, dev)
    thresholds = (_f32(max_grad), _f32(pc.percent_dense * extent), _f32(min_opacity), 1 if max_screen_size else 0,
                  _f32(max_screen_size) if max_screen_size else 0.0, _f32(0.1 * extent))

    def plan(ws, totals, stream):
        return _lib.r3dgs_densify_plan(P, 1, pc.xyz_gradient_accum.data_ptr(), pc.denom.data_ptr(), pc._scaling.data_ptr(),
                                       pc._opacity.data_ptr(), pc.max_radii2D.data_ptr(), *thresholds, ws, totals, stream)
    totals = _run(what, pc, entries, P, dev, plan, noise, zero_accumulators=True)
    densification_statistics_dict["n_points_pruned"] = totals[6]
    densification_statistics_dict["n_points_cloned"] = totals[4]
    densification_statistics_dict["n_points_split"] = totals[5]


def prune(pc, min_opacity, extent, max_screen_size, densification_statistics_dict, store_grads=False):
    """GaussianModel.prune (scene/gaussian_model.py:684-691) called on its own: the screen-size term sees max_radii2D as it
    is, and the three accumulators are compacted with the parameters."""
    what = "prune"
    P, dev, entries = ms.collect(what, pc, _CHILD_KIND, ZERO_NEW, store_grads, accumulators=True)
    thresholds = (1.0, 0.0, _f32(min_opacity), 1 if max_screen_size else 0, _f32(max_screen_size) if max_screen_size else 0.0,
                  _f32(0.1 * extent))

    def plan(ws, totals, stream):
        return _lib.r3dgs_densify_plan(P, 0, None, None, pc._scaling.data_ptr(), pc._opacity.data_ptr(),
                                       pc.max_radii2D.data_ptr(), *thresholds, ws, totals, stream)
    totals = _run(what, pc, entries, P, dev, plan, None, zero_accumulators=False)
    densification_statistics_dict["n_points_pruned"] = totals[6]


def prune_points(pc, mask, store_grads=False):
    """GaussianModel.prune_points (scene/gaussian_model.py:553-568): removes the Gaussians with mask True.  mask: bool [P] on
    the device (what mercy_points builds in torch)."""
    what = "prune_points"
    P = ms.model_size(what, pc)
    ms.check_extra(what, "mask", mask, torch.bool, (P,), f"(P,) with P = {P}")
    P, dev, entries = ms.collect(what, pc, _CHILD_KIND, ZERO_NEW, store_grads, accumulators=True)
    ms.check_extra_device(what, "mask", mask, dev)

    def plan(ws, totals, stream):
        return _lib.r3dgs_prune_plan(P, mask.data_ptr(), ws, totals, stream)
    _run(what, pc, entries, P, dev, plan, None, zero_accumulators=False)
