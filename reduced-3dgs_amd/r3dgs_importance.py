"""Per-Gaussian blend-contribution scores over a camera set (include/r3dgs_importance.h, csrc/importance.hip): how much each
Gaussian contributes to the rendered pixels, the quantity contribution-based pruning ranks by.

For one view, with w = alpha * T the blend weight of a Gaussian at a pixel that blends it and an optional pixel weight map m:
    sum    sum of m * w over the pixels with m != 0            (float64)
    max    the largest w over those pixels                     (float32, at most 0.99)
    count  the number of those pixels                          (int64)
    views  the views in which count > 0                        (int32)
Over a camera set sum and count add up, max is the maximum.  A pixel of weight 0 is left out of everything, so a 0/1 map lifts a
2D mask to the Gaussians it selects and an error map against the ground truth weights the sum by where the render is wrong.

What the score is NOT: it is not the reference's redundancy score (reduction_ops / calculate_redundancy_metric: voxel overlap
and opacity, no rendering), it carries no gradient, and a low score says "little seen from THESE cameras", not "useless".

    scores = contribution_scores(cameras, model, pipe, background)
    r3dgs_densify.prune_points(model, low_contribution_mask(scores, keep_fraction=0.6))

Each view is rendered under torch.no_grad() and scored by one native call over the state that forward left; nothing in the
loop waits for the device.  `model` is a GaussianModel-shaped object or a r3dgs_quantised.QuantisedModel.
"""
import math

import torch

from diff_gaussian_rasterization import Scores, _C, new_scores
from diff_gaussian_rasterization import contribution_scores as _native_scores

__all__ = ["Scores", "view_scores", "contribution_scores", "low_contribution_mask"]


def _model_size(model):
    P = getattr(model, "P", None)
    return int(P) if P is not None else int(model._xyz.shape[0])


def _checked_weight(what, pixel_weight, H, W, dev):
    """The refusals of a pixel weight map, before anything is launched -> the map as the native call takes it."""
    if pixel_weight is None:
        return None
    if not isinstance(pixel_weight, torch.Tensor) or tuple(pixel_weight.shape[-2:]) != (H, W) or pixel_weight.numel() != H * W:
        shape = tuple(pixel_weight.shape) if isinstance(pixel_weight, torch.Tensor) else type(pixel_weight).__name__
        raise ValueError(f"{what}: pixel_weight must be an [H, W] = [{H}, {W}] tensor, got {shape}")
    if pixel_weight.dtype != torch.float32:
        raise ValueError(f"{what}: pixel_weight must be float32, got {str(pixel_weight.dtype)[6:]}")
    if pixel_weight.device != dev:
        raise ValueError(f"{what}: pixel_weight must live on {dev}, got {pixel_weight.device}")
    if not pixel_weight.is_contiguous():
        raise ValueError(f"{what}: pixel_weight must be contiguous")
    return pixel_weight.detach()


def _checked_out(what, out, P, dev):
    if out is None:
        return
    if not isinstance(out, Scores):
        raise ValueError(f"{what}: out must be a Scores (diff_gaussian_rasterization.new_scores), got {type(out).__name__}")
    for name, t in out._asdict().items():
        if tuple(t.shape) != (P,) or t.dtype != _C._SCORE_DTYPES[name] or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{what}: out.{name} must be a contiguous {str(_C._SCORE_DTYPES[name])[6:]} [{P}] tensor on {dev}, "
                             f"got {str(t.dtype)[6:]} {tuple(t.shape)} on {t.device}")


def _score_view(what, camera, model, pipe, background, weight_of, out, accumulate, render):
    """One view: render, then one native call over the state the forward left.  weight_of(render_pkg) -> the weight map."""
    P = _model_size(model)
    H, W = int(camera.image_height), int(camera.image_width)
    with torch.no_grad():
        with _C.forward_state() as st:
            pkg = render(camera, model, pipe, background)
        weight = _checked_weight(what, weight_of(pkg), H, W, background.device)
        if st.result is None:   # an empty model: nothing was rendered
            return out if accumulate else _native_scores(P, 0, H, W, *([torch.empty(0, dtype=torch.uint8, device=background.device)] * 3),
                                                         pixel_weight=weight, out=out)
        num_rendered, _, radii, geom, binning, img = st.result
        return _native_scores(int(radii.numel()), num_rendered, H, W, geom, binning, img, pixel_weight=weight, out=out,
                              accumulate=accumulate)


def view_scores(camera, model, pipe, background, *, pixel_weight=None, out=None, render=None):
    """The scores of ONE view -> Scores (written into `out`, a Scores, when given: overwritten, not accumulated).  The view is
    rendered under torch.no_grad() with r3dgs_render.render (or `render`, same signature); pixel_weight: float32 [H, W] on the
    device or None."""
    what = "view_scores"
    if render is None:
        from r3dgs_render import render
    if not isinstance(background, torch.Tensor) or not background.is_cuda:
        raise RuntimeError(f"{what}: background is a host tensor; the scores need device tensors (no CPU path)")
    H, W = int(camera.image_height), int(camera.image_width)
    _checked_weight(what, pixel_weight, H, W, background.device)
    _checked_out(what, out, _model_size(model), background.device)
    return _score_view(what, camera, model, pipe, background, lambda pkg: pixel_weight, out, False, render)


def contribution_scores(cameras, model, pipe, background, *, pixel_weights=None, render=None):
    """The scores of `model` over every camera of `cameras`, accumulated on the device -> Scores.  pixel_weights: None, a
    sequence of one [H, W] float32 map (or None) per camera, or a callable (index, camera, render_pkg) -> such a map (for
    example the per-pixel error of render_pkg["render"] against camera.original_image).  Nothing in the loop waits for the
    device; the caller decides when to read."""
    what = "contribution_scores"
    if render is None:
        from r3dgs_render import render
    cameras = list(cameras)
    if not cameras:
        raise ValueError(f"{what}: no cameras")
    if not isinstance(background, torch.Tensor) or not background.is_cuda:
        raise RuntimeError(f"{what}: background is a host tensor; the scores need device tensors (no CPU path)")
    if pixel_weights is not None and not callable(pixel_weights):
        pixel_weights = list(pixel_weights)
        if len(pixel_weights) != len(cameras):
            raise ValueError(f"{what}: {len(pixel_weights)} pixel weight maps for {len(cameras)} cameras")
        for camera, m in zip(cameras, pixel_weights):   # (before anything is launched)
            _checked_weight(what, m, int(camera.image_height), int(camera.image_width), background.device)
    total = new_scores(_model_size(model), background.device)
    for v, camera in enumerate(cameras):
        if pixel_weights is None:
            weight_of = lambda pkg: None   # noqa: E731
        elif callable(pixel_weights):
            weight_of = lambda pkg, v=v, camera=camera: pixel_weights(v, camera, pkg)   # noqa: E731
        else:
            weight_of = lambda pkg, v=v: pixel_weights[v]   # noqa: E731
        _score_view(what, camera, model, pipe, background, weight_of, total, True, render)
    return total


def low_contribution_mask(scores, *, max_below=None, sum_below=None, keep_fraction=None, never_seen=True):
    """A bool [P] mask of the Gaussians to REMOVE (what r3dgs_densify.prune_points(pc, mask) takes): those whose largest blend
    weight is below `max_below`, or whose sum is below `sum_below`, or that are not among the ceil(keep_fraction * P) largest
    sums (torch.topk) -- whichever of the three are given; asking for none is refused.  never_seen=True: a Gaussian no counted
    pixel blended is in the mask as well; never_seen=False: it is left out of the mask whatever its (zero) scores say -- the
    cameras may simply not have looked at it.  No host wait."""
    what = "low_contribution_mask"
    if not isinstance(scores, Scores):
        raise ValueError(f"{what}: scores must be a Scores, got {type(scores).__name__}")
    if max_below is None and sum_below is None and keep_fraction is None:
        raise ValueError(f"{what}: name a criterion: max_below, sum_below or keep_fraction")
    P = int(scores.sum.shape[0])
    mask = torch.zeros(P, dtype=torch.bool, device=scores.sum.device)
    if max_below is not None:
        mask |= scores.max < float(max_below)
    if sum_below is not None:
        mask |= scores.sum < float(sum_below)
    if keep_fraction is not None:
        if not 0.0 < float(keep_fraction) <= 1.0:
            raise ValueError(f"{what}: keep_fraction = {keep_fraction!r} must lie in (0, 1]")
        k = min(P, int(math.ceil(float(keep_fraction) * P)))
        drop = torch.ones(P, dtype=torch.bool, device=scores.sum.device)
        if k:
            drop.scatter_(0, torch.topk(scores.sum, k).indices, False)   # (an indexed assignment would wait for the device)
        mask |= drop
    unseen = scores.count == 0
    return (mask | unseen) if never_seen else (mask & ~unseen)
