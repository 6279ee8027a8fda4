"""diff_gaussian_rasterization -- MI355X-native drop-in for the rasterizer package of
graphdeco-inria/reduced-3dgs (submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py).

Public surface kept identical so that gaussian_renderer.render(), train.py and render.py run unmodified:
`GaussianRasterizationSettings` (12 fields, same order, :169-181), `GaussianRasterizer(raster_settings)`
with `.forward(...)` / `.markVisible(...)` (:183-234), `rasterize_gaussians(...)` and the autograd
function `_RasterizeGaussians` (:21-167), plus the `_C` operator module.

Put `reduced-3dgs_amd/` on PYTHONPATH (before or instead of the CUDA submodule) to switch a reference
checkout over.  Behavioural notes:
  * the reference hard-codes debug=True in the forward call (:85), i.e. a device synchronisation after
    every stage; here `raster_settings.debug` is honoured.  debug=False (what render() passes) takes the
    asynchronous path: nothing waits for num_rendered, a pass is one hipGraph launch, and `ctx.num_rendered`
    is an int-like `_C.NumRendered` that is only fetched from the device if somebody looks at it;
    debug=True takes the exact-size path with a synchronisation after every stage;
  * gradients are bit-reproducible: the backward has no float atomics (the reference issues one per
    (pixel, Gaussian, component), so its low bits depend on scheduling).
"""
import contextlib
import functools
import threading
import weakref
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def cpu_deep_copy_tuple(input_tuple):
    """Host snapshot of an argument tuple, written out if the native call fails in debug mode."""
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _call_native(fn, args, debug, dump_name):
    if not debug:
        return fn(*args)
    snapshot = cpu_deep_copy_tuple(args)  # taken before the call so a crash cannot corrupt it
    try:
        return fn(*args)
    except Exception:
        torch.save(snapshot, dump_name)
        print(f"\nAn error occured in the rasterizer. Inputs were written to {dump_name} for debugging.")
        raise


# ---- absolute screen-space gradients (AbsGS; gsplat's absgrad): see absgrad() -----------------------------------------------
# The request travels beside the autograd functions' inputs and the public signatures (which are the reference's): a scope
# (absgrad()) or a one-shot note (rasterize_gaussians(..., absgrad=True)), taken by the forwards issued on the same thread.
class _AbsgradRequest(threading.local):
    on = scope = False   # per thread; the class attributes are what a thread that never asked reads


_absgrad_request = _AbsgradRequest()


@contextlib.contextmanager
def absgrad(on=True):
    """Renders issued inside `with absgrad():` -- GaussianRasterizer(...)(...), rasterize_gaussians, rasterize_gaussian_params,
    on this thread -- also return the absolute screen-space gradients: after backward(), the `means2D` tensor passed to the
    render carries `means2D.absgrad`, a detached float32 [P,3] tensor: per Gaussian the sum over its pixels of the ABSOLUTE
    value of what each pixel adds to means2D.grad (include/r3dgs_rasterizer.h r3dgs_backward_absgrad), third column zero (the
    gsplat convention).  It is OVERWRITTEN, not accumulated, by each backward of that render.  Every other result of the render
    and of its backward is what it is outside the scope, bit for bit.  A render that needs no gradient asks for nothing."""
    before = _absgrad_request.scope
    _absgrad_request.scope = bool(on)
    try:
        yield
    finally:
        _absgrad_request.scope = before


def _ask_absgrad(on):
    _absgrad_request.on = bool(on)


def _take_absgrad(ctx, means2D):
    """In a forward: whether the render asked for the abs gradients -> ctx.absgrad_target (a weak reference to the caller's
    means2D tensor, or None).  Nothing is asked of a render that needs no gradient."""
    req = _absgrad_request
    if not (req.on or req.scope):   # the usual case: one attribute set
        ctx.absgrad_target = None
        return
    req.on = False   # the one-shot note is taken
    ctx.absgrad_target = weakref.ref(means2D) if any(ctx.needs_input_grad) else None


def _abs_native(ctx, native):
    return functools.partial(native, _absgrad=True) if ctx.absgrad_target is not None else native


def _split_absgrad(ctx, out):
    """A native backward's result without its trailing dL_dmeans2D_abs, which becomes `.absgrad` of the render's means2D."""
    out = tuple(out)
    if ctx.absgrad_target is None:
        return out
    target = ctx.absgrad_target()
    if target is not None:
        target.absgrad = out[-1]
    return out[:-1]


class _RasterizeGaussians(torch.autograd.Function):
    """Autograd boundary of the tile rasterizer.  Inputs (positional, as the reference):
    means3D, means2D, sh, degrees, colors_precomp, opacities (raw), scales (activated), rotations (unit),
    cov3Ds_precomp, raster_settings, lambda_sh_sparsity  ->  (color[3,H,W], radii[P])."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, degrees, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, lambda_sh_sparsity):
        rs = raster_settings
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, degrees,
                rs.campos, rs.prefiltered, rs.debug)
        _C.hint_next_forward(any(ctx.needs_input_grad))   # rendering under no_grad: nothing is kept for a backward's sake
        _take_absgrad(ctx, means2D)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _call_native(
            _C.rasterize_gaussians, args, rs.debug, "snapshot_fw.dump")
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.lambda_sh_sparsity = lambda_sh_sparsity
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                              binningBuffer, imgBuffer, degrees)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)  # no zeros_like(radii) fill per backward for the non-differentiable output
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer,
         degrees) = ctx.saved_tensors
        if grad_out_color is None:  # the image did not take part in the loss
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=means3D.dtype,
                                         device=means3D.device)
        args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, degrees, rs.campos,
                geomBuffer, ctx.num_rendered, binningBuffer, imgBuffer, ctx.lambda_sh_sparsity, rs.debug)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations) = (_call_native(_C.rasterize_gaussians_backward, args, rs.debug, "snapshot_bw.dump")
                            if ctx.absgrad_target is None else
                            _split_absgrad(ctx, _call_native(_abs_native(ctx, _C.rasterize_gaussians_backward), args, rs.debug,
                                                             "snapshot_bw.dump")))
        # one slot per forward input; None for degrees, raster_settings, lambda_sh_sparsity
        return (grad_means3D, grad_means2D, grad_sh, None, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp, None, None)


def rasterize_gaussians(means3D, means2D, sh, degrees, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, lambda_sh_sparsity, absgrad=False):
    """absgrad=True: this render as inside `with absgrad():` -- after backward(), `means2D.absgrad` holds its absolute
    screen-space gradients (float32 [P,3], detached, third column zero; overwritten, not accumulated, by each backward of it)."""
    _ask_absgrad(absgrad)
    return _RasterizeGaussians.apply(means3D, means2D, sh, degrees, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, lambda_sh_sparsity)


class _RasterizeGaussianParams(torch.autograd.Function):
    """Autograd boundary of the rasterizer fed with the model's RAW parameters, as the reference's GaussianModel stores
    them: xyz, means2D, features_dc [P,1,3], features_rest [P,M-1,3], degrees, opacity (raw), scaling (log), rotation
    (unnormalised), raster_settings, lambda_sh_sparsity  ->  (color[3,H,W], radii[P]).  exp / normalize / cat happen inside
    the kernels; the backward hands the library's outputs straight back as the gradients of these tensors."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, degrees, opacity, scaling, rotation, raster_settings,
                lambda_sh_sparsity):
        rs = raster_settings
        args = (rs.bg, xyz, features_dc, features_rest, degrees, opacity, scaling, rotation, rs.scale_modifier, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.campos, rs.prefiltered, rs.debug)
        _C.hint_next_forward(any(ctx.needs_input_grad))
        _take_absgrad(ctx, means2D)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _call_native(
            _C.rasterize_gaussian_params, args, rs.debug, "snapshot_fw.dump")
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.lambda_sh_sparsity = lambda_sh_sparsity
        ctx.save_for_backward(xyz, features_dc, features_rest, degrees, opacity, scaling, rotation, radii, geomBuffer,
                              binningBuffer, imgBuffer)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        rs = ctx.raster_settings
        (xyz, features_dc, features_rest, degrees, opacity, scaling, rotation, radii, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors
        if grad_out_color is None:  # the image did not take part in the loss
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=xyz.dtype, device=xyz.device)
        args = (rs.bg, xyz, radii, features_dc, features_rest, degrees, opacity, scaling, rotation, rs.scale_modifier,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, rs.campos, geomBuffer,
                ctx.num_rendered, binningBuffer, imgBuffer, ctx.lambda_sh_sparsity, rs.debug)
        (grad_means2D, grad_opacity, grad_xyz, grad_dc, grad_rest, grad_scaling, grad_rotation) = (
            _call_native(_C.rasterize_gaussian_params_backward, args, rs.debug, "snapshot_bw.dump")
            if ctx.absgrad_target is None else
            _split_absgrad(ctx, _call_native(_abs_native(ctx, _C.rasterize_gaussian_params_backward), args, rs.debug,
                                             "snapshot_bw.dump")))
        if features_rest.numel() == 0:
            grad_rest = None
        # one slot per forward input; None for degrees, raster_settings, lambda_sh_sparsity
        return (grad_xyz, grad_means2D, grad_dc, grad_rest, None, grad_opacity, grad_scaling, grad_rotation, None, None)


def rasterize_gaussian_params(xyz, means2D, features_dc, features_rest, degrees, opacity, scaling, rotation, raster_settings,
                              lambda_sh_sparsity=0.):
    """The rasterizer from GaussianModel's raw tensors (_xyz, _features_dc, _features_rest, _degrees, _opacity, _scaling,
    _rotation) -> (color, radii); gradients flow to exactly those tensors.  (Inside `with absgrad():` as GaussianRasterizer.)"""
    if features_rest is None:
        features_rest = torch.Tensor([])
    rs = raster_settings
    if _camera_requires_grad(rs):   # a camera tensor asks for a gradient: the camera-differentiable function
        return _RasterizeGaussianParamsCam.apply(xyz, means2D, features_dc, features_rest, degrees, opacity, scaling, rotation,
                                                 rs, lambda_sh_sparsity, rs.viewmatrix, rs.projmatrix, rs.campos)
    return _RasterizeGaussianParams.apply(xyz, means2D, features_dc, features_rest, degrees, opacity, scaling, rotation,
                                          raster_settings, lambda_sh_sparsity)


def _camera_requires_grad(rs):
    """True if one of the settings' three camera tensors asks for a gradient (under grad mode)."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                           for t in (rs.viewmatrix, rs.projmatrix, rs.campos))


# ---- the camera-differentiable pair.  Each is its existing counterpart plus three inputs (viewmatrix, projmatrix, campos) and
# one more call in the backward; what the two share lives in the helpers below, the originals are not touched. ----------------

def _cam_settings(raster_settings, model_device, viewmatrix, projmatrix, campos):
    """raster_settings with the three camera tensors as the native calls read them -- detached, contiguous -- checked HERE,
    before the forward is issued: the camera pass reads them in place and would refuse them only in the backward."""
    for name, t, numel in (("viewmatrix", viewmatrix, 16), ("projmatrix", projmatrix, 16), ("campos", campos, 3)):
        if not isinstance(t, torch.Tensor) or t.numel() != numel:
            raise RuntimeError(f"camera gradients: {name} must be a tensor of {numel} elements")
        if t.device != model_device:
            raise RuntimeError(f"camera gradients: {name}: expected a tensor on {model_device}, got {t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"camera gradients: {name}: expected float32, got {str(t.dtype)[6:]}")
    return raster_settings._replace(viewmatrix=viewmatrix.detach().contiguous(), projmatrix=projmatrix.detach().contiguous(),
                                    campos=campos.detach().contiguous())


def _cam_forward(ctx, native, args, rs, lambda_sh_sparsity, saved, means2D):
    """The forward body of both functions: the native call `native(*args)`, the context, `saved(radii, geomBuffer,
    binningBuffer, imgBuffer)` -> the tensors to keep.  means2D: the caller's tensor (where an abs gradient would go)."""
    _C.hint_next_forward(any(ctx.needs_input_grad))
    _take_absgrad(ctx, means2D)
    num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _call_native(native, args, rs.debug, "snapshot_fw.dump")
    ctx.raster_settings, ctx.num_rendered, ctx.lambda_sh_sparsity = rs, num_rendered, lambda_sh_sparsity
    ctx.save_for_backward(*saved(radii, geomBuffer, binningBuffer, imgBuffer))
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)
    return color, radii


def _cam_upstream(rs, grad_out_color, like):
    if grad_out_color is None:  # the image did not take part in the loss
        return torch.zeros((3, rs.image_height, rs.image_width), dtype=like.dtype, device=like.device)
    return grad_out_color


def _cam_backward(ctx, first_camera_slot, native, args, raw, **model):
    """The native backward `native(*args)`, asked for its per-Gaussian sums as well -- its result starts with dL_dmeans2D and
    ends with (dL_dcolors, dL_dconic) -- then the camera pass for the camera inputs that need a gradient (they are the inputs
    first_camera_slot .. + 2 of the function) -> (native's result, the three camera slots).  **model: camera_backward's
    model arguments."""
    rs = ctx.raster_settings
    got = _split_absgrad(ctx, _call_native(native, args, rs.debug, "snapshot_bw.dump"))
    needs = ctx.needs_input_grad[first_camera_slot:first_camera_slot + 3]
    want = tuple(n for n, need in zip(_C.CAMERA_GRADS, needs) if need)
    cam = {}
    if want:
        cam = _C.camera_backward(scale_modifier=rs.scale_modifier, raw_params=raw, viewmatrix=rs.viewmatrix, projmatrix=rs.projmatrix,
                                 campos=rs.campos, tanfovx=rs.tanfovx, tanfovy=rs.tanfovy, image_height=rs.image_height,
                                 image_width=rs.image_width, dL_dmeans2D=got[0], dL_dcolors=got[-2], dL_dconic=got[-1], want=want,
                                 **model)
    return got, tuple(cam.get(n) for n in _C.CAMERA_GRADS)


class _RasterizeGaussiansCam(torch.autograd.Function):
    """_RasterizeGaussians with the camera differentiable.  Inputs: those of _RasterizeGaussians, then viewmatrix [4,4],
    projmatrix [4,4], campos [3] -- the tensors of raster_settings, handed in as arguments so that autograd sees them.
    The forward is the same native call; the backward is the same native backward, asked for its per-Gaussian dL_dconic as
    well, followed by `_C.camera_backward` for the camera tensors that need a gradient.  The three are independent inputs:
    what ties them together (a pose) is chained by autograd outside (r3dgs_camera.RefinedCamera)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, degrees, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, lambda_sh_sparsity, viewmatrix, projmatrix, campos):
        rs = _cam_settings(raster_settings, means3D.device, viewmatrix, projmatrix, campos)
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, degrees,
                rs.campos, rs.prefiltered, rs.debug)
        return _cam_forward(ctx, _C.rasterize_gaussians, args, rs, lambda_sh_sparsity,
                            lambda radii, geom, binning, img: (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii,
                                                               sh, geom, binning, img, degrees), means2D)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer,
         degrees) = ctx.saved_tensors
        args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, _cam_upstream(rs, grad_out_color, means3D), sh, degrees,
                rs.campos, geomBuffer, ctx.num_rendered, binningBuffer, imgBuffer, ctx.lambda_sh_sparsity, rs.debug)

        want_abs = ctx.absgrad_target is not None

        def native(*a):   # -> the eight gradients, then (dL_dcolors again, dL_dconic); an empty model has no conic rows
            out = tuple(_C.rasterize_gaussians_backward(*a, _want_conic=True, _absgrad=want_abs))
            tail = out[-1:] if want_abs else ()   # dL_dmeans2D_abs stays last
            out = out[:-1] if want_abs else out
            return out[:8] + (out[1], out[8] if len(out) == 9 else None) + tail
        got, cam = _cam_backward(ctx, 11, native, args, False, means3D=means3D, degrees=degrees,
                                 sh=None if colors_precomp.numel() else sh, sh_rest=None, scales=scales, rotations=rotations,
                                 cov3D_precomp=cov3Ds_precomp, radii=radii, geomBuffer=geomBuffer)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations) = got[:8]
        return (grad_means3D, grad_means2D, grad_sh, None, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp, None, None) + cam


class _RasterizeGaussianParamsCam(torch.autograd.Function):
    """_RasterizeGaussianParams with the camera differentiable: its inputs, then viewmatrix, projmatrix, campos (see
    _RasterizeGaussiansCam).  The per-Gaussian kernel of the camera pass activates the raw scaling / rotation itself."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, degrees, opacity, scaling, rotation, raster_settings,
                lambda_sh_sparsity, viewmatrix, projmatrix, campos):
        rs = _cam_settings(raster_settings, xyz.device, viewmatrix, projmatrix, campos)
        args = (rs.bg, xyz, features_dc, features_rest, degrees, opacity, scaling, rotation, rs.scale_modifier, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.campos, rs.prefiltered, rs.debug)
        return _cam_forward(ctx, _C.rasterize_gaussian_params, args, rs, lambda_sh_sparsity,
                            lambda radii, geom, binning, img: (xyz, features_dc, features_rest, degrees, opacity, scaling, rotation,
                                                               radii, geom, binning, img), means2D)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        rs = ctx.raster_settings
        (xyz, features_dc, features_rest, degrees, opacity, scaling, rotation, radii, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors
        args = (rs.bg, xyz, radii, features_dc, features_rest, degrees, opacity, scaling, rotation, rs.scale_modifier,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, _cam_upstream(rs, grad_out_color, xyz), rs.campos, geomBuffer,
                ctx.num_rendered, binningBuffer, imgBuffer, ctx.lambda_sh_sparsity, rs.debug)
        no_rest = features_rest.numel() == 0
        want_abs = ctx.absgrad_target is not None
        got, cam = _cam_backward(ctx, 10, lambda *a: _C.rasterize_gaussian_params_backward(*a, _want_2d=True, _absgrad=want_abs),
                                 args, True,
                                 means3D=xyz, degrees=degrees, sh=features_dc, sh_rest=None if no_rest else features_rest,
                                 scales=scaling, rotations=rotation, cov3D_precomp=None, radii=radii, geomBuffer=geomBuffer)
        grad_means2D, grad_opacity, grad_xyz, grad_dc, grad_rest, grad_scaling, grad_rotation = got[:7]
        return (grad_xyz, grad_means2D, grad_dc, None if no_rest else grad_rest, None, grad_opacity, grad_scaling, grad_rotation,
                None, None) + cam


def aux_maps(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer,
             maps=("depth", "alpha", "median_depth")):
    """Per-pixel maps replayed from the three buffers a forward returned (`_C.rasterize_gaussians*` hand them out; P is the
    model's size, num_rendered the forward's first result) -> {name: float [1,H,W]} for the names in `maps`:
      "depth"         sum over the blended Gaussians of z * alpha * T (view depth z; fp32, list order).  Not normalised, no
                      background term: divide by "alpha" for a mean depth
      "alpha"         1 - final transmittance
      "median_depth"  z of the first blended Gaussian after which T < 0.5; 0 where none brings T below 0.5
    and 0 in all three where nothing contributed.  One kernel launch, no host wait; the buffers are only read, so a backward
    over them afterwards is unaffected.  The maps carry NO gradient."""
    with torch.no_grad():
        return _C.aux_maps(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, maps=maps)


class Scores(NamedTuple):
    """Per-Gaussian blend-contribution scores, each [P]: `sum` (float64) of pixel_weight * alpha * T over the pixels that blend
    the Gaussian, `max` (float32) of alpha * T, `count` (int64) of those pixels, `views` (int32) of the views with count > 0."""
    sum: torch.Tensor
    max: torch.Tensor
    count: torch.Tensor
    views: torch.Tensor


def new_scores(P, device):
    """Zeroed buffers for `contribution_scores(..., out=..., accumulate=True)`."""
    return Scores(*(torch.zeros(int(P), dtype=_C._SCORE_DTYPES[name], device=device) for name in _C.SCORES))


def contribution_scores(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, pixel_weight=None,
                        out=None, accumulate=False):
    """How much each Gaussian contributed to the pixels of the view whose forward left the three buffers (include/
    r3dgs_importance.h) -> Scores.  pixel_weight: float32 [H, W] on the device or None (ones); a pixel of weight 0 is left out
    of every score, so a 0/1 map is a region of interest and an error map weights the sum.  out: a Scores to write in place
    (None: a new one); accumulate=True folds the view into it (sum and count add, max is the maximum, views counts the views
    that saw the Gaussian) instead of overwriting it.  No host wait, no float atomics, the same bits from run to run; the
    buffers are only read, so a backward over them afterwards is unaffected."""
    if out is not None and not isinstance(out, Scores):
        raise ValueError(f"contribution_scores: out must be a Scores, got {type(out).__name__}")
    with torch.no_grad():
        got = _C.contribution_scores(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer,
                                     pixel_weight=pixel_weight, out=None if out is None else out._asdict(),
                                     accumulate=accumulate)
    return out if out is not None else Scores(*(got[name] for name in _C.SCORES))


def aux_maps_backward(*args, **kwargs):
    """Thin wrapper of `_C.aux_maps_backward` (include/r3dgs_aux.h r3dgs_aux_maps_backward): the gradients of the maps of
    `aux_maps` with respect to the Gaussians, from upstream gradients of the maps, over the same three buffers."""
    with torch.no_grad():
        return _C.aux_maps_backward(*args, **kwargs)


# ---- the three replay maps with gradients (_AuxMaps, _DistortionMap, _FeatureMaps) share what they save and their backward
# The six model tensors in autograd's input order.  The native calls name the same six as _C.AUX_GRADS, which puts means2D
# first; the mapping between the two orders is by NAME, below, never by position.
_MODEL_INPUTS = ("means3D", "means2D", "opacity", "scales", "rotations", "cov3D")
assert sorted(_MODEL_INPUTS) == sorted(_C.AUX_GRADS)


def _replay_call(native, state, rs, *args, **kwargs):
    """native(P, num_rendered, H, W, the three buffers of the forward's six-tuple `state`, ...)."""
    num_rendered, _, radii, geomBuffer, binningBuffer, imgBuffer = state
    return native(int(radii.numel()), num_rendered, rs.image_height, rs.image_width, geomBuffer, binningBuffer, imgBuffer, *args,
                  **kwargs)


def _replay_save(ctx, state, rs, means3D, scales, rotations, cov3D_precomp, *more):
    """What _replay_backward reads, then the unit's own tensors `more` (ctx.saved_tensors[8:])."""
    ctx.raster_settings, ctx.num_rendered = rs, state[0]
    ctx.save_for_backward(means3D, scales, rotations, cov3D_precomp, *state[2:], *more)


def _replay_backward(ctx, native, names, *upstream):
    """One native backward asked for the gradients autograd wants.  names: the function's leading inputs that can take one,
    by the native call's names; upstream: that call's arguments behind radii."""
    rs = ctx.raster_settings
    means3D, scales, rotations, cov3D_precomp, radii, geomBuffer, binningBuffer, imgBuffer = ctx.saved_tensors[:8]
    want = tuple(n for n, need in zip(names, ctx.needs_input_grad) if need)
    got = native(int(radii.numel()), ctx.num_rendered, rs.image_height, rs.image_width, geomBuffer, binningBuffer, imgBuffer,
                 rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, means3D, scales, rs.scale_modifier, rotations,
                 cov3D_precomp, radii, *upstream, want=want)
    return tuple(got.get(n) for n in names) + (None,) * (len(ctx.needs_input_grad) - len(names))


def _or_empty(*tensors):
    """The optional scales / rotations / cov3D_precomp as an autograd function takes them: an empty tensor for None."""
    return tuple(torch.Tensor([]) if t is None else t for t in tensors)


class _AuxMaps(torch.autograd.Function):
    """`aux_maps` with gradients.  Inputs: means3D, means2D, opacities (raw), scales (activated), rotations (unit),
    cov3D_precomp (or an empty tensor), then without gradient: the forward's six-tuple `state` (num_rendered, color, radii,
    geomBuffer, binningBuffer, imgBuffer), raster_settings and the names of the maps  ->  one [1,H,W] tensor per name.
    The forward is `aux_maps`; the backward is `aux_maps_backward` over the saved buffers."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings, maps):
        got = _replay_call(_C.aux_maps, state, raster_settings, maps=maps)
        ctx.maps = tuple(maps)
        _replay_save(ctx, state, raster_settings, means3D, scales, rotations, cov3D_precomp)
        ctx.set_materialize_grads(False)
        return tuple(got[name] for name in maps)

    @staticmethod
    def backward(ctx, *grads):
        up = dict(zip(ctx.maps, grads))
        return _replay_backward(ctx, _C.aux_maps_backward, _MODEL_INPUTS, up.get("depth"), up.get("alpha"), up.get("median_depth"))


def aux_maps_with_grad(means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings,
                       maps=("depth", "alpha", "median_depth")):
    """The maps of `aux_maps` ATTACHED to the model's tensors -> {name: float [1,H,W]}.  `state`: the six-tuple the forward
    returned (what `_C.forward_state()` records); scales / rotations: the activated values the forward saw (or cov3D_precomp);
    means2D: the screen-space tensor whose .grad densification reads -- it receives the maps' share as well."""
    maps = tuple(maps)
    got = _AuxMaps.apply(means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state, raster_settings, maps)
    return dict(zip(maps, got))


def distortion_map(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, near=0.0, far=0.0):
    """The depth-distortion map (the squared form of the 2DGS regulariser) replayed from the three buffers a forward returned
    -> float [1,H,W]: per pixel sum_{j<k} w_j w_k (m_k - m_j)^2 over the Gaussians the forward blended, w = alpha T, m the
    mapped depth -- m = z for near = far = 0, 2DGS's m = far / (far - near) (1 - near / z) for 0 < near < far.  No background
    term, 0 where nothing contributed.  One kernel launch, no host wait; the buffers are only read.  The map carries NO
    gradient (`distortion_map_with_grad` attaches it)."""
    with torch.no_grad():
        return _C.distortion_map(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, near, far)


class _DistortionMap(torch.autograd.Function):
    """`distortion_map` with gradients.  Inputs as `_AuxMaps`: means3D, means2D, opacities (raw), scales (activated), rotations
    (unit), cov3D_precomp (or an empty tensor), then without gradient: the forward's six-tuple `state`, raster_settings and the
    (near, far) pair  ->  the [1,H,W] map.  The backward is `_C.distortion_map_backward` over the saved buffers and moments."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings, mapping):
        ctx.mapping = _C.depth_mapping(mapping)
        out, moments = _replay_call(_C.distortion_map, state, raster_settings, *ctx.mapping, want_moments=True)
        _replay_save(ctx, state, raster_settings, means3D, scales, rotations, cov3D_precomp, moments)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, grad):
        return _replay_backward(ctx, _C.distortion_map_backward, _MODEL_INPUTS, grad, ctx.saved_tensors[8], *ctx.mapping)


def distortion_map_with_grad(means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings,
                             near=0.0, far=0.0):
    """The map of `distortion_map` ATTACHED to the model's tensors -> float [1,H,W].  Arguments as `aux_maps_with_grad`;
    means2D receives the map's share of the screen-space gradient as well."""
    return _DistortionMap.apply(means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state, raster_settings,
                                (near, far))


def feature_maps(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, features):
    """A per-Gaussian feature vector blended into a map, replayed from the three buffers a forward returned: features float32
    [P, C] -> float [C, H, W], map[c] = sum over the blended Gaussians of features[id, c] * alpha * T (fp32, list order).  Not
    normalised, no background term: divide by the "alpha" map of `aux_maps` for a mean.  One kernel launch, no host wait; the
    buffers are only read, so a backward over them afterwards is unaffected.  The map is detached (`feature_maps_with_grad`
    carries gradients)."""
    with torch.no_grad():
        return _C.feature_maps(P, num_rendered, image_height, image_width, geomBuffer, binningBuffer, imgBuffer, features)


def feature_maps_backward(*args, **kwargs):
    """Thin wrapper of `_C.feature_maps_backward` (include/r3dgs_features.h r3dgs_feature_maps_backward)."""
    with torch.no_grad():
        return _C.feature_maps_backward(*args, **kwargs)


class _FeatureMaps(torch.autograd.Function):
    """`feature_maps` with gradients.  Inputs: features [P, C], then the model's tensors as `_AuxMaps` takes them -- means3D,
    means2D, opacities (raw), scales (activated), rotations (unit), cov3D_precomp (or an empty tensor); pass tensors that do
    not require grad (detached) for a frozen geometry -- then without gradient: the forward's six-tuple `state` and
    raster_settings  ->  the [C, H, W] map.  The backward is one `feature_maps_backward` over the saved buffers, asked only
    for the gradients autograd wants."""

    @staticmethod
    def forward(ctx, features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings):
        out = _replay_call(_C.feature_maps, state, raster_settings, features)
        _replay_save(ctx, state, raster_settings, means3D, scales, rotations, cov3D_precomp, features)
        return out   # (no set_materialize_grads(False) here, unlike the two above)

    @staticmethod
    def backward(ctx, grad_out):
        return _replay_backward(ctx, _C.feature_maps_backward, ("features",) + _MODEL_INPUTS, ctx.saved_tensors[8], grad_out)


def feature_maps_with_grad(features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings):
    """The map of `feature_maps` ATTACHED to `features` and to whichever of the model's tensors require grad -> float
    [C, H, W].  `state`: the six-tuple the forward returned (what `_C.forward_state()` records); scales / rotations: the
    activated values the forward saw (or cov3D_precomp); means2D: the screen-space tensor whose .grad densification reads."""
    return _FeatureMaps.apply(features, means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state,
                              raster_settings)


# ---- the three replay maps with the camera differentiable as well (_AuxMapsCam, _DistortionMapCam, _FeatureMapsCam).  Each is
# its counterpart above plus two inputs (viewmatrix, projmatrix, LAST, as _RasterizeGaussiansCam has them) and, in the backward,
# the map's _screen call followed by a camera pass of its own (_C.camera_backward_maps); autograd adds the shares of the maps
# and of the colour route.  There is no campos input: no SH direction is involved. ---------------------------------------------

def _cam_map_settings(raster_settings, model_device, viewmatrix, projmatrix):
    """raster_settings with the two camera tensors as the native calls read them -- detached, contiguous -- checked in the
    forward: the camera pass reads them in place and would refuse them only in the backward."""
    for name, t in (("viewmatrix", viewmatrix), ("projmatrix", projmatrix)):
        if not isinstance(t, torch.Tensor) or t.numel() != 16:
            raise RuntimeError(f"camera gradients of the maps: {name} must be a tensor of 16 elements")
        if t.device != model_device:
            raise RuntimeError(f"camera gradients of the maps: {name}: expected a tensor on {model_device}, got {t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"camera gradients of the maps: {name}: expected float32, got {str(t.dtype)[6:]}")
    return raster_settings._replace(viewmatrix=viewmatrix.detach().contiguous(), projmatrix=projmatrix.detach().contiguous())


def _replay_backward_cam(ctx, native, names, *upstream):
    """_replay_backward for a function whose last two inputs are viewmatrix and projmatrix: where one of them needs a gradient
    the native call is its _screen form, asked for the screen-space sums as well, and `_C.camera_backward_maps` turns those into
    the two partial derivatives.  A model none of whose tensors needs a gradient (a tracker) is not differentiated at all."""
    rs = ctx.raster_settings
    means3D, scales, rotations, cov3D_precomp, radii, geomBuffer, binningBuffer, imgBuffer = ctx.saved_tensors[:8]
    needs = ctx.needs_input_grad
    want = tuple(n for n, need in zip(names, needs) if need)
    cam_want = tuple(n for n, need in zip(_C.CAMERA_MAP_GRADS, needs[-2:]) if need)
    screen = ("means2D",) + _C.SCREEN_GRADS
    got = native(int(radii.numel()), ctx.num_rendered, rs.image_height, rs.image_width, geomBuffer, binningBuffer, imgBuffer,
                 rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, means3D, scales, rs.scale_modifier, rotations,
                 cov3D_precomp, radii, *upstream, want=want + tuple(n for n in screen if cam_want and n not in want),
                 _screen=bool(cam_want))
    cam = {}
    if cam_want:
        cam = _C.camera_backward_maps(means3D, scales, rotations, rs.scale_modifier, cov3D_precomp, rs.viewmatrix, rs.projmatrix,
                                      rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, radii, got["means2D"],
                                      got["conic"], got["z"], want=cam_want)
    return (tuple(got[n] if n in want else None for n in names) + (None,) * (len(needs) - len(names) - 2)
            + tuple(cam.get(n) for n in _C.CAMERA_MAP_GRADS))


class _AuxMapsCam(torch.autograd.Function):
    """_AuxMaps with the camera differentiable: its inputs, then viewmatrix [4,4] and projmatrix [4,4] -- the tensors of
    raster_settings, handed in as arguments so that autograd sees them.  The backward is `_C.aux_maps_backward_screen` and
    `_C.camera_backward_maps`; the two are independent inputs, chained outside (r3dgs_camera.RefinedCamera)."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings, maps, viewmatrix,
                projmatrix):
        rs = _cam_map_settings(raster_settings, means3D.device, viewmatrix, projmatrix)
        return _AuxMaps.forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, rs, maps)

    @staticmethod
    def backward(ctx, *grads):
        up = dict(zip(ctx.maps, grads))
        return _replay_backward_cam(ctx, _C.aux_maps_backward, _MODEL_INPUTS, up.get("depth"), up.get("alpha"),
                                    up.get("median_depth"))


class _DistortionMapCam(torch.autograd.Function):
    """_DistortionMap with the camera differentiable: its inputs, then viewmatrix and projmatrix (see _AuxMapsCam).  The
    backward is `_C.distortion_backward_screen` and `_C.camera_backward_maps`."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings, mapping, viewmatrix,
                projmatrix):
        rs = _cam_map_settings(raster_settings, means3D.device, viewmatrix, projmatrix)
        return _DistortionMap.forward(ctx, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, rs, mapping)

    @staticmethod
    def backward(ctx, grad):
        return _replay_backward_cam(ctx, _C.distortion_map_backward, _MODEL_INPUTS, grad, ctx.saved_tensors[8], *ctx.mapping)


class _FeatureMapsCam(torch.autograd.Function):
    """_FeatureMaps with the camera differentiable: its inputs, then viewmatrix and projmatrix (see _AuxMapsCam).  The
    backward is `_C.feature_maps_backward_screen` and `_C.camera_backward_maps`."""

    @staticmethod
    def forward(ctx, features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings, viewmatrix,
                projmatrix):
        rs = _cam_map_settings(raster_settings, means3D.device, viewmatrix, projmatrix)
        return _FeatureMaps.forward(ctx, features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, rs)

    @staticmethod
    def backward(ctx, grad_out):
        return _replay_backward_cam(ctx, _C.feature_maps_backward, ("features",) + _MODEL_INPUTS, ctx.saved_tensors[8], grad_out)


def aux_maps_with_camera_grad(means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings,
                              maps=("depth", "alpha", "median_depth")):
    """`aux_maps_with_grad` whose maps are attached to raster_settings.viewmatrix / .projmatrix as well."""
    maps = tuple(maps)
    rs = raster_settings
    got = _AuxMapsCam.apply(means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state, rs, maps,
                            rs.viewmatrix, rs.projmatrix)
    return dict(zip(maps, got))


def distortion_map_with_camera_grad(means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings,
                                    near=0.0, far=0.0):
    """`distortion_map_with_grad` whose map is attached to raster_settings.viewmatrix / .projmatrix as well."""
    rs = raster_settings
    return _DistortionMapCam.apply(means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state, rs,
                                   (near, far), rs.viewmatrix, rs.projmatrix)


def feature_maps_with_camera_grad(features, means3D, means2D, opacities, scales, rotations, cov3D_precomp, state, raster_settings):
    """`feature_maps_with_grad` whose map is attached to raster_settings.viewmatrix / .projmatrix as well."""
    rs = raster_settings
    return _FeatureMapsCam.apply(features, means3D, means2D, opacities, *_or_empty(scales, rotations, cov3D_precomp), state, rs,
                                 rs.viewmatrix, rs.projmatrix)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """bool[P]: which positions pass the near-plane test of this camera (view-space z > 0.2)."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, degrees=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None, lambda_sh_sparsity=0.):
        """(The parameters are the reference's.  Called inside `with diff_gaussian_rasterization.absgrad():`, the backward of
        this render also leaves `means2D.absgrad` on the means2D tensor passed in -- see absgrad().)"""
        if (shs is None) == (colors_precomp is None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        has_sr = scales is not None or rotations is not None
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (has_sr and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        # absent optional inputs travel as empty tensors (-> NULL at the C ABI), like the reference
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        rs = self.raster_settings
        if _camera_requires_grad(rs):   # a camera tensor asks for a gradient: the camera-differentiable function
            return _RasterizeGaussiansCam.apply(means3D, means2D, shs, degrees, colors_precomp, opacities, scales, rotations,
                                                cov3D_precomp, rs, lambda_sh_sparsity, rs.viewmatrix, rs.projmatrix, rs.campos)
        return rasterize_gaussians(means3D, means2D, shs, degrees, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, self.raster_settings, lambda_sh_sparsity)
