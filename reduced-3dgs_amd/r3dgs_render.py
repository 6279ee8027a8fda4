"""r3dgs_render -- `render()` with the keyword surface and result dictionary of the reference's
gaussian_renderer.render, rasterizing straight from the model's raw parameters when it can.

The reference's render() activates the model in torch on every call -- exp(_scaling), F.normalize(_rotation),
cat(_features_dc, _features_rest) -- and autograd undoes it again in the backward (slices of the joined SH gradient copied
into the two parameters' .grad).  Here the rasterizer's per-Gaussian kernels apply the activations and read / write SH as
the two tensors the model stores (diff_gaussian_rasterization.rasterize_gaussian_params), so none of that glue runs.

    from r3dgs_render import render          # instead of: from gaussian_renderer import render

The fused path is taken when the call asks for nothing it does not cover; otherwise -- pipe.compute_cov3D_python,
pipe.convert_SHs_python, override_color, variable_sh_bands -- the call does what the reference's does, through the existing
package entry points.  `pc` is anything shaped like the reference's GaussianModel: _xyz, _features_dc, _features_rest,
_opacity, _scaling, _rotation, _degrees, active_sh_degree, max_sh_degree (and get_* / get_covariance / per_band_count for
the fallback routes) -- or a r3dgs_quantised.QuantisedModel, which is rendered from its ids and codebooks in place
(the three Python-side options, override_color and lambda_sh_sparsity are refused).  A QuantisedModel on which gradients
were asked for (`requires_grad_`) trains, with grad enabled, through the same raw-parameter route on tensors decoded for the
step, and the result then carries "viewspace_points" like any model's; otherwise "viewspace_points" is None.

`aux=("depth", "alpha", "median_depth")` (or any subset) adds those keys to the result: float [1,H,W] maps replayed from the
state the forward left (diff_gaussian_rasterization.aux_maps, include/r3dgs_aux.h) -- "depth" is the blend-weighted sum of
the view depths (NOT normalised: divide by "alpha" for a mean), "alpha" = 1 - final transmittance, "median_depth" the depth of
the first Gaussian that brings the transmittance below 0.5 (0 where none does).  One extra kernel launch per call; by default the
maps carry no gradient (detached tensors), and the backward of "render" is what it is without them.  aux=None (the default): no
extra launch, the same keys as before.

`aux_grad=True` (with `aux`, under grad mode, for a model with something trainable -- a ValueError otherwise) returns the maps
ATTACHED to the model's tensors instead: a loss on "depth" / "alpha" / "median_depth" reaches xyz, opacity, scaling and rotation
(and the codebooks of a trainable QuantisedModel) through diff_gaussian_rasterization._AuxMaps, whose backward is one
r3dgs_aux_maps_backward over the forward's state; its gradients add to those of "render" through autograd, and
"viewspace_points".grad receives both.  On the raw-parameter route and for a QuantisedModel the activated scales and rotations
the function takes are built in torch (pc.get_scaling / pc.get_rotation) only in this case, so torch carries the gradient
through exp / normalize and the decode.  "median_depth" hands its gradient to the depth of the Gaussian it selected.

Camera gradients.  A camera whose world_view_transform, full_proj_transform or camera_center is a tensor that requires grad
(r3dgs_camera.RefinedCamera builds such a camera from a 6-parameter pose correction) makes "render" differentiable with respect
to those tensors too, on the raw-parameter route and on the activated one: the backward runs one more pass over the Gaussians
(include/r3dgs_camera.h) and autograd chains the three partial derivatives through whatever ties the tensors together.  Refused
with a ValueError: a QuantisedModel, and -- unless camera_grad_maps=True -- aux_grad=True, distortion and features_geom_grad=True.
tan_fov / the focal length is not differentiated.

`camera_grad_maps=True` (with a camera that requires grad; a no-op otherwise) carries the maps' share of a pose gradient: the
maps of aux_grad=True, distortion= and features_geom_grad=True are attached to world_view_transform / full_proj_transform as well
as to whatever in the model is trainable (diff_gaussian_rasterization._AuxMapsCam / _DistortionMapCam / _FeatureMapsCam: the
map's _screen backward, then include/r3dgs_camera.h r3dgs_camera_backward_maps), and autograd adds their shares to the colour
route's.  The model may be frozen in this mode -- a tracker: only the camera gets gradients, and the "nothing trainable" refusal
does not apply.  Still refused: normals=True, antialiasing=True and a QuantisedModel with a camera that requires grad.

`features=F` (float32 [P, C] on the model's device, 1 <= C <= _C.FEATURE_MAX_CHANNELS; a non-contiguous F is made contiguous)
adds the key "features": the [C,H,W] map sum F[id] alpha T over the blended Gaussians (include/r3dgs_features.h) -- not
normalised and without a background term, like "depth".  One extra launch on the forward's state instead of ceil(C / 3) renders
with colors_precomp = F[:, c:c+3].  If F requires grad the map is attached to F (diff_gaussian_rasterization._FeatureMaps; the
geometry stays frozen and the backward skips its sums); `features_geom_grad=True` attaches it to the model's geometry as well,
and those gradients add to the colour backward's through autograd ("viewspace_points".grad receives both).  `pc` may be a
QuantisedModel.  Refused with a ValueError: features_geom_grad=True for a QuantisedModel, together with a camera that requires
grad (unless camera_grad_maps=True), or under no_grad; an F of the wrong shape, dtype, device or channel count.  `features` combines freely with `aux` /
`aux_grad`; features=None (the default): the same dictionary, no extra launch, no recorder.

Anti-aliasing.  `antialiasing=True` multiplies every Gaussian's opacity by rho = sqrt(det C / det(C + 0.3 I)) of its projected
covariance in this view (the official rasterizer's `antialiasing`, gsplat's "antialiased" mode with eps2d = 0.3 -- not
Mip-Splatting's 0.1 kernel); `filter_3d=f` (float32 [P,1] from r3dgs_mip.filter_3d) applies Mip-Splatting's 3D smoothing filter
to the scales and opacities.  Both are differentiable maps from raw parameters to raw parameters (r3dgs_mip,
include/r3dgs_mip.h) placed in front of the unchanged rasterizer: the model is rendered through a thin view whose _scaling /
_opacity are the filtered tensors -- the 3D filter first, the 2D compensation on its result -- and autograd composes the maps'
backward with the rasterizer's.  Every route, `aux`, `aux_grad`, `features` and `features_geom_grad` work unchanged.  With both
off (the default) nothing new is launched.  Refused with a ValueError: a QuantisedModel; filter_3d with
pipe.compute_cov3D_python; antialiasing=True with a camera that requires grad; an f of the wrong shape, dtype or device.

Surface normals.  `normals=True` adds the key "normal": the [3,H,W] map sum n_i alpha T of the Gaussians' view-space normals
(r3dgs_normals.gaussian_normals: the axis of the smallest scale, turned towards the camera), blended by the feature-map launch
over the forward's state -- together with `features=F` the three channels ride the same launch (C + 3 <=
_C.FEATURE_MAX_CHANNELS).  Not normalised, like "depth" and "features".  Under grad mode the map is attached to the model's
rotation through the normals' own backward, and with `features_geom_grad=True` to the geometry through the blend weights, as a
user-supplied F would be; on the raw-parameter route the raw tensors go in.  `antialiasing` / `filter_3d` combine unchanged
(the 3D filter adds the same term to all three squared scales: the smallest stays the smallest).  r3dgs_normals.
normal_consistency(out["normal"], out["depth"], rs, alpha=out["alpha"]) is the depth-normal consistency loss.  normals=False
(the default): the same dictionary, nothing new is launched, no recorder.  Refused with a ValueError before anything is
launched: a QuantisedModel, pipe.compute_cov3D_python (no axis to pick), a camera that requires grad.

Depth distortion.  `distortion=True` or `distortion=(near, far)` adds the key "distortion": the [1,H,W] map sum_{j<k} w_j w_k
(m_k - m_j)^2 over the Gaussians the forward blended, w = alpha T (include/r3dgs_distortion.h: the squared form 2DGS's
rasterizer computes; the linear-order form of Mip-NeRF 360 / gsplat is not offered).  True: the mapped depth m is the view depth
z; (near, far) with 0 < near < far: 2DGS's m = far / (far - near) (1 - near / z).  One extra launch on the forward's state.
Under grad mode, for a model with something trainable, the map is attached to the model's tensors
(diff_gaussian_rasterization._DistortionMap) and "viewspace_points".grad receives its share, as with `aux_grad`; otherwise --
no_grad, nothing trainable, a QuantisedModel -- it is detached.  The 2DGS recipe: lambda_dist * out["distortion"].mean() next
to r3dgs_normals.normal_consistency.  It combines with `aux`, `aux_grad`, `features`, `normals`, `antialiasing` and `filter_3d`
on every route; distortion=None / False (the default): the same dictionary, nothing new is launched.  Refused with a
ValueError before anything is launched: a trainable QuantisedModel under grad mode, a camera that requires grad (unless camera_grad_maps=True), a (near, far)
that is neither (0, 0) nor 0 < near < far.

Absolute screen-space gradients (AbsGS; gsplat's absgrad).  `absgrad=True`: after backward(), out["viewspace_points"].absgrad is a
detached float32 [P,3] tensor -- per Gaussian, the sum over its pixels of the ABSOLUTE value of what each pixel adds to
"viewspace_points".grad (columns 0 and 1; column 2 is zero, rows of culled Gaussians are zero).  It comes out of the backward
blend itself (include/r3dgs_rasterizer.h r3dgs_backward_absgrad): every gradient, the image and the radii are what they are
without the keyword, bit for bit.  It describes the COLOUR loss's backward only: `aux_grad`, `features_geom_grad`, `normals` and
`distortion` add their terms to "viewspace_points".grad through autograd and nothing to .absgrad.  It is OVERWRITTEN, not
accumulated, by each backward of this render.  Works on every route that has a backward (raw-parameter, activated, a camera
that requires grad, a trainable QuantisedModel) and with `antialiasing` / `filter_3d`; under no_grad, or for a model that needs no
gradient, it is a no-op.  r3dgs_train_stats.add_densification_stats_absgrad(pc, viewspace_points, radii) feeds it to the densifiers.
absgrad=False (the default): nothing new is launched.
"""
import functools
import inspect
import math
import threading

import torch

from diff_gaussian_rasterization import (GaussianRasterizationSettings, GaussianRasterizer, _C, aux_maps,
                                         aux_maps_with_camera_grad, aux_maps_with_grad, distortion_map,
                                         distortion_map_with_camera_grad, distortion_map_with_grad, feature_maps,
                                         feature_maps_with_camera_grad, feature_maps_with_grad, rasterize_gaussian_params)
from diff_gaussian_rasterization import absgrad as absgrad_scope
from r3dgs_quantised import QuantisedModel

# render(aux_grad=True) asks the call it wraps for the tensors its forward was fed: a dictionary here, for the duration of that
# call, receives "inputs" = (means3D, opacities, scales, rotations, cov3D_precomp) -- what _AuxMaps differentiates with respect
# to.  Routes that built the activated values anyway hand those over; the others build them only when asked.
_tls = threading.local()


def _hand_over(means3D, opacities, scales, rotations, cov3D_precomp):
    want = getattr(_tls, "inputs", None)
    if want is not None:
        want["inputs"] = (means3D, opacities, scales() if callable(scales) else scales,
                          rotations() if callable(rotations) else rotations, cov3D_precomp)


def _settings(camera, pc, pipe, bg_color, scaling_modifier):
    return GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width),
        tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=camera.camera_center, prefiltered=False, debug=bool(pipe.debug))


def camera_requires_grad(camera):
    """True when, under grad mode, one of the camera's world_view_transform / full_proj_transform / camera_center is a tensor
    that requires grad: render() then differentiates the image with respect to them as well (the module's docstring)."""
    if camera is None or not torch.is_grad_enabled():
        return False
    return any(isinstance(t, torch.Tensor) and t.requires_grad
               for t in (getattr(camera, n, None) for n in ("world_view_transform", "full_proj_transform", "camera_center")))


def fused_path_applies(pc, pipe, override_color=None, variable_sh_bands=False):
    """True when render() will rasterize from the raw parameters: nothing precomputed in Python, dense SH, and parameter
    tensors the kernels can read in place (float32, contiguous)."""
    if override_color is not None or variable_sh_bands or pipe.compute_cov3D_python or pipe.convert_SHs_python:
        return False
    tensors = (pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation)
    return all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def _render_quantised(camera, qm, pipe, bg_color, scaling_modifier, override_color, lambda_sh_sparsity, measure_fps):
    """render() of a QuantisedModel.  Inference (no_grad, or nobody asked for gradients): the rasterizer reads ids, positions
    and codebooks in place.  Training: decode for this step, the raw-parameter route, the lookup's adjoint in the backward."""
    if override_color is not None:
        raise ValueError("render: override_color is not supported for a QuantisedModel (colours come from its codebooks); "
                         "decode() it and render the dense tensors")
    if pipe.compute_cov3D_python:
        raise ValueError("render: pipe.compute_cov3D_python is not supported for a QuantisedModel (the kernels activate the "
                         "looked-up scales and rotations); decode() it and render the dense tensors")
    if pipe.convert_SHs_python:
        raise ValueError("render: pipe.convert_SHs_python is not supported for a QuantisedModel (the kernels evaluate SH from "
                         "the ids); decode() it and render the dense tensors")
    if lambda_sh_sparsity:
        raise ValueError("render: the SH-sparsity term is not available for a QuantisedModel (lambda_sh_sparsity must be 0)")
    rs = _settings(camera, qm, pipe, bg_color, scaling_modifier)
    fps = 0
    if measure_fps:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
    if qm.trainable and torch.is_grad_enabled():
        xyz, dc, rest, opacity, scaling, rotation, degrees = qm.decode_for_training()
        _hand_over(xyz, opacity, lambda: torch.exp(scaling), lambda: torch.nn.functional.normalize(rotation), None)
        screenspace_points = torch.zeros_like(xyz, requires_grad=True) + 0
        screenspace_points.retain_grad()
        image, radii = rasterize_gaussian_params(xyz, screenspace_points, dc, rest, degrees, opacity, scaling, rotation, rs, 0.)
        if measure_fps:
            t1.record()
            torch.cuda.synchronize()
            fps = 1 / t0.elapsed_time(t1)
        return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
                "FPS": fps}
    _, image, radii, _, _, _ = _C.rasterize_gaussians_quantised(
        rs.bg, qm.xyz, qm.geom_ids, qm.sh_ids, qm.codebooks, rs.scale_modifier, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
        rs.tanfovy, rs.image_height, rs.image_width, qm.per_band, qm.cumsum, qm.coeffs, rs.campos, rs.prefiltered, rs.debug)
    if measure_fps:
        t1.record()
        torch.cuda.synchronize()
        fps = 1 / t0.elapsed_time(t1)
    return {"render": image, "viewspace_points": None, "visibility_filter": radii > 0, "radii": radii, "FPS": fps}


def _with_aux(aux, camera, out, state):
    """`out` with the maps named in `aux` added, from the six-tuple `state` of the forward that produced it (None: an empty
    model, nothing was rendered -- zero maps)."""
    H, W = int(camera.image_height), int(camera.image_width)
    if state is None:
        dev = out["render"].device
        out.update({name: torch.zeros((1, H, W), dtype=torch.float32, device=dev) for name in aux})
        return out
    num_rendered, _, radii, geom, binning, img = state
    with torch.no_grad():
        out.update(aux_maps(int(radii.numel()), num_rendered, H, W, geom, binning, img, maps=aux))
    return out


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None, lambda_sh_sparsity=0.,
           measure_fps=False, variable_sh_bands=False):
    """Render the scene seen by `viewpoint_camera`.  bg_color must be a device tensor.
    -> {"render", "viewspace_points", "visibility_filter", "radii", "FPS"}
    Keyword-only extension (not a parameter of the reference's render, so not part of this signature): aux=("depth", "alpha",
    "median_depth") or any subset adds those maps, each float [1,H,W] without gradient; see the module's docstring."""
    if isinstance(pc, QuantisedModel):
        return _render_quantised(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, lambda_sh_sparsity,
                                 measure_fps)
    xyz = pc._xyz
    # a zero tensor whose gradient is the screen-space gradient of the means (densification statistics)
    screenspace_points = torch.zeros_like(xyz, requires_grad=True) + 0
    try:
        screenspace_points.retain_grad()
    except Exception:
        pass
    rs = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    fused = fused_path_applies(pc, pipe, override_color, variable_sh_bands)

    if not fused:
        scales = rotations = cov3D_precomp = shs = colors_precomp = None
        if pipe.compute_cov3D_python:
            cov3D_precomp = pc.get_covariance(scaling_modifier)
        else:
            scales, rotations = pc.get_scaling, pc.get_rotation
        if override_color is not None:
            colors_precomp = override_color
        elif pipe.convert_SHs_python:
            from utils.sh_utils import eval_sh   # the training repository's own SH evaluation
            feats = pc.get_features
            shs_view = feats.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dirs = pc.get_xyz - viewpoint_camera.camera_center.repeat(feats.shape[0], 1)
            dirs = dirs / dirs.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dirs) + 0.5, 0.0)
        else:
            shs = pc.get_features
            if variable_sh_bands:   # the ragged, degree-sorted buffer of the inference path
                shs = torch.cat([t.flatten() for t in shs])

    fps = 0
    if measure_fps:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
    if fused:
        image, radii = rasterize_gaussian_params(xyz, screenspace_points, pc._features_dc, pc._features_rest, pc._degrees,
                                                 pc._opacity, pc._scaling, pc._rotation, rs, lambda_sh_sparsity)
    elif variable_sh_bands:
        dev = xyz.device
        per_band = torch.tensor(pc.per_band_count, device=dev, dtype=torch.int)
        cumsum = torch.cumsum(per_band, dim=0).to(dtype=torch.int)
        coeffs = torch.tensor([i * i for i in range(1, len(pc.per_band_count) + 1)], device=dev, dtype=torch.int)
        none = torch.Tensor([])
        _, image, radii, _, _, _ = _C.rasterize_gaussians_variableSH_bands(
            rs.bg, pc.get_xyz, none, pc._opacity, scales, rotations, rs.scale_modifier, none, rs.viewmatrix, rs.projmatrix,
            rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, shs, per_band, cumsum, coeffs, pc._degrees, rs.campos,
            rs.prefiltered, rs.debug)
    else:
        image, radii = GaussianRasterizer(raster_settings=rs)(
            means3D=pc.get_xyz, means2D=screenspace_points, shs=shs, degrees=pc._degrees, colors_precomp=colors_precomp,
            opacities=pc._opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp,
            lambda_sh_sparsity=lambda_sh_sparsity)
    if measure_fps:
        t1.record()
        torch.cuda.synchronize()
        fps = 1 / t0.elapsed_time(t1)
    if fused:   # the kernels activated the raw parameters: torch's own activations, only if somebody asks
        _hand_over(xyz, pc._opacity, lambda: pc.get_scaling if hasattr(pc, "get_scaling") else torch.exp(pc._scaling),
                   lambda: pc.get_rotation if hasattr(pc, "get_rotation") else torch.nn.functional.normalize(pc._rotation), None)
    else:
        _hand_over(pc.get_xyz, pc._opacity, scales, rotations, cov3D_precomp)

    # culled Gaussians (radius 0) take no part in the densification statistics
    return {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "FPS": fps}


_render = render   # the reference's signature, parameter for parameter (tests/test_params_cpu.py holds it to the reference's source)


def _checked_features(features, pc, features_geom_grad, camera, cam_maps=False):
    """The refusals of render(features=...), before anything is launched."""
    P = int(pc.P) if isinstance(pc, QuantisedModel) else int(pc._xyz.shape[0])
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != P:
        shape = tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__
        raise ValueError(f"render: features must be a [P, C] tensor with P = {P} rows (one per Gaussian), got {shape}")
    if not 1 <= features.shape[1] <= _C.FEATURE_MAX_CHANNELS:
        raise ValueError(f"render: features needs 1 <= C <= {_C.FEATURE_MAX_CHANNELS} channels, got C = {features.shape[1]}")
    if features.dtype != torch.float32:
        raise ValueError(f"render: features must be float32, got {str(features.dtype)[6:]}")
    where = pc.xyz.device if isinstance(pc, QuantisedModel) else pc._xyz.device
    if features.device.type != "cuda" or features.device != where:
        raise ValueError(f"render: features must live on the model's device ({where}), got {features.device}")
    if features_geom_grad:
        _checked_geom_grad(pc, camera, cam_maps)


def _checked_geom_grad(pc, camera, cam_maps=False):
    """The refusals of render(features_geom_grad=True)."""
    if isinstance(pc, QuantisedModel):
        raise ValueError("render: features_geom_grad=True is not available for a QuantisedModel (geometry gradients of its "
                         "codebooks through the feature map are out of scope); its features alone can be trained")
    if camera_requires_grad(camera) and not cam_maps:
        raise ValueError("render: features_geom_grad=True together with a camera that requires grad is not supported: the "
                         "feature map's share of a pose gradient is out of scope (camera_grad_maps=True carries it)")
    if not torch.is_grad_enabled():
        raise ValueError("render: features_geom_grad=True under no_grad: there is no graph to attach the map to")


def _anchored(zero, tensors):
    """An empty model's map: `zero`, attached to those of `tensors` that require grad (a backward through it is valid and
    leaves zero gradients)."""
    return zero + 0.0 * sum(t.sum() for t in tensors if t is not None and t.requires_grad)


def _feature_map(features, camera, out, state, rs, inputs=None, cam_maps=False):
    """The "features" entry of the result: [C,H,W] from the six-tuple `state` of the forward that produced `out` (None: an empty
    model -- a zero map), attached to `features` when it requires grad and, with `inputs` (means3D, opacities, scales,
    rotations, cov3D_precomp), to the model's geometry as well."""
    H, W = int(camera.image_height), int(camera.image_width)
    attach = torch.is_grad_enabled() and (features.requires_grad or inputs is not None)
    if state is None:
        zero = torch.zeros((features.shape[1], H, W), dtype=torch.float32, device=out["render"].device)
        return _anchored(zero, (features,)) if attach and features.requires_grad else zero
    if not attach:
        num_rendered, _, radii, geom, binning, img = state
        return feature_maps(int(radii.numel()), num_rendered, H, W, geom, binning, img, features)
    if inputs is None:   # frozen geometry: the backward skips the geometric sums and reads none of the model's tensors
        empty = torch.Tensor([])
        return feature_maps_with_grad(features, empty, empty, empty, None, None, None, state, rs)
    means3D, opacities, scales, rotations, cov3D = inputs
    attached = feature_maps_with_camera_grad if cam_maps else feature_maps_with_grad
    return attached(features, means3D, out["viewspace_points"], opacities, scales, rotations, cov3D, state, rs)


def _distortion_map(mapping, camera, out, state, rs, inputs, cam_maps=False):
    """The "distortion" entry of the result: [1,H,W] from the six-tuple `state` of the forward that produced `out` (None: an
    empty model -- a zero map); with `inputs` (means3D, opacities, scales, rotations, cov3D_precomp) attached to them."""
    H, W = int(camera.image_height), int(camera.image_width)
    near, far = mapping
    if state is None:
        zero = torch.zeros((1, H, W), dtype=torch.float32, device=out["render"].device)
        return zero if inputs is None else _anchored(zero, inputs)
    if inputs is None:
        num_rendered, _, radii, geom, binning, img = state
        return distortion_map(int(radii.numel()), num_rendered, H, W, geom, binning, img, near, far)
    means3D, opacities, scales, rotations, cov3D = inputs
    attached = distortion_map_with_camera_grad if cam_maps else distortion_map_with_grad
    return attached(means3D, out["viewspace_points"], opacities, scales, rotations, cov3D, state, rs, near, far)


_SIGNATURE = inspect.signature(_render)


class _FilteredModel:
    """A thin view of a model whose _scaling / _opacity are the anti-aliased tensors: everything else is the model's own.
    The activated getters follow the two tensors, so every route of render() -- all of them read RAW opacity -- sees them."""

    def __init__(self, pc, scaling, opacity):
        self.__dict__.update(_pc=pc, _scaling=scaling, _opacity=opacity)

    def __getattr__(self, name):   # only reached for what the view does not hold itself
        return getattr(self._pc, name)

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)


def _checked_filter_3d(filter_3d, pc):
    """The refusals of render(filter_3d=...): shape, dtype, device."""
    P = int(pc._xyz.shape[0])
    if not isinstance(filter_3d, torch.Tensor) or tuple(filter_3d.shape) != (P, 1):
        shape = tuple(filter_3d.shape) if isinstance(filter_3d, torch.Tensor) else type(filter_3d).__name__
        raise ValueError(f"render: filter_3d must be a [P, 1] tensor with P = {P} (r3dgs_mip.filter_3d), got {shape}")
    if filter_3d.dtype != torch.float32:
        raise ValueError(f"render: filter_3d must be float32, got {str(filter_3d.dtype)[6:]}")
    if filter_3d.device.type != "cuda" or filter_3d.device != pc._xyz.device:
        raise ValueError(f"render: filter_3d must live on the model's device ({pc._xyz.device}), got {filter_3d.device}")


def _antialiased_model(camera, pc, pipe, bg_color, scaling_modifier, antialiasing, filter_3d):
    """The model render(antialiasing=..., filter_3d=...) rasterizes: the refusals first (before anything is launched), then
    the 3D filter on the raw parameters and the per-view 2D compensation on its result (r3dgs_mip)."""
    import r3dgs_mip
    if isinstance(pc, QuantisedModel):
        raise ValueError("render: antialiasing / filter_3d are not available for a QuantisedModel (its opacity and scaling live "
                         "in codebooks); decode() it and render the dense tensors")
    if filter_3d is not None and pipe.compute_cov3D_python:
        raise ValueError("render: filter_3d together with pipe.compute_cov3D_python is not supported (the model's own "
                         "get_covariance would not see the filtered scaling)")
    if antialiasing and camera_requires_grad(camera):
        raise ValueError("render: antialiasing=True together with a camera that requires grad is not supported: rho depends on "
                         "the view and its share of a pose gradient is out of scope")
    if filter_3d is not None:
        _checked_filter_3d(filter_3d, pc)
    scaling, opacity = pc._scaling, pc._opacity
    if filter_3d is not None:
        scaling, opacity = r3dgs_mip.filtered_parameters(scaling, opacity, filter_3d)
    if antialiasing:
        rs = _settings(camera, pc, pipe, bg_color, scaling_modifier)
        if pipe.compute_cov3D_python:
            opacity = r3dgs_mip.antialias_opacity(pc.get_xyz, opacity, None, None, pc.get_covariance(scaling_modifier), rs)
        else:
            opacity = r3dgs_mip.antialias_opacity(pc._xyz, opacity, scaling, pc._rotation, None, rs, raw=True)
    return _FilteredModel(pc, scaling, opacity)


def _checked_normals(camera, pc, pipe, features):
    """The refusals of render(normals=True), before anything is launched."""
    if isinstance(pc, QuantisedModel):
        raise ValueError("render: normals=True is not available for a QuantisedModel (its scales and rotations live in "
                         "codebooks); decode() it and render the dense tensors")
    if pipe.compute_cov3D_python:
        raise ValueError("render: normals=True together with pipe.compute_cov3D_python is not supported (a precomputed "
                         "covariance has no axis to pick)")
    if camera_requires_grad(camera):
        raise ValueError("render: normals=True together with a camera that requires grad is not supported: the normals' share "
                         "of a pose gradient is out of scope")
    if isinstance(features, torch.Tensor) and features.dim() == 2 and features.shape[1] + 3 > _C.FEATURE_MAX_CHANNELS:
        raise ValueError(f"render: normals=True rides the feature launch: C + 3 <= {_C.FEATURE_MAX_CHANNELS} channels, got "
                         f"C = {features.shape[1]}")


def _model_normals(pc, pipe, rs, override_color, variable_sh_bands):
    """The [P,3] view-space normals render(normals=True) blends: from the raw tensors where render() rasterizes from them."""
    import r3dgs_normals
    if fused_path_applies(pc, pipe, override_color, variable_sh_bands):
        return r3dgs_normals.gaussian_normals(pc._xyz.detach(), pc._scaling.detach(), pc._rotation, rs, raw=True)
    return r3dgs_normals.gaussian_normals(pc.get_xyz.detach(), pc.get_scaling.detach(), pc.get_rotation, rs, raw=False)


@functools.wraps(_render)
def render(*args, aux=None, **kwargs):
    if kwargs.pop("absgrad", False):   # likewise: out["viewspace_points"].absgrad after backward (the module's docstring)
        with absgrad_scope():   # every rasterizer forward this render issues asks for them
            return render(*args, aux=aux, **kwargs)
    aux_grad = bool(kwargs.pop("aux_grad", False))   # keyword on top of `aux` (the module's docstring); default: today's maps
    features = kwargs.pop("features", None)          # likewise: the [P, C] tensor of the "features" map; default: no such key
    features_geom_grad = bool(kwargs.pop("features_geom_grad", False))
    antialiasing = bool(kwargs.pop("antialiasing", False))   # likewise: the two anti-aliasing filters (the module's docstring);
    filter_3d = kwargs.pop("filter_3d", None)                # both off: today's path, nothing new is launched
    normals = bool(kwargs.pop("normals", False))             # likewise: the "normal" map (the module's docstring)
    distortion = kwargs.pop("distortion", None)              # likewise: the "distortion" map; None / False: no such key
    mapping = None if distortion is None or distortion is False else _C.depth_mapping(distortion)
    camera_grad_maps = bool(kwargs.pop("camera_grad_maps", False))   # likewise: the maps' share of a pose gradient
    camera = args[0] if args else kwargs.get("viewpoint_camera")
    if callable(getattr(camera, "snapshot", None)):   # a camera that builds its tensors on access (r3dgs_camera.RefinedCamera):
        camera = camera.snapshot()                    # built once for this render
        if args:
            args = (camera,) + tuple(args[1:])
        else:
            kwargs["viewpoint_camera"] = camera
    if antialiasing or filter_3d is not None:
        b = _SIGNATURE.bind(*args, **kwargs)
        b.apply_defaults()
        b.arguments["pc"] = _antialiased_model(camera, b.arguments["pc"], b.arguments["pipe"], b.arguments["bg_color"],
                                               b.arguments["scaling_modifier"], antialiasing, filter_3d)
        args, kwargs = b.args, b.kwargs
    # the maps attached to the camera's tensors as well (a no-op for a camera that does not require grad)
    cam_maps = camera_grad_maps and camera_requires_grad(camera)
    if camera_requires_grad(camera):   # (before anything is launched)
        pc = args[1] if len(args) > 1 else kwargs.get("pc")
        if isinstance(pc, QuantisedModel):
            raise ValueError("render: camera gradients are not available for a QuantisedModel (its forward reads ids and "
                             "codebooks; no backward of it writes the per-Gaussian sums they are formed from); decode() it and "
                             "render the dense tensors")
        if aux_grad and not cam_maps:
            raise ValueError("render: aux_grad=True together with a camera that requires grad is not supported: the maps' "
                             "share of a pose gradient is out of scope (render the maps without aux_grad, or detach the camera; "
                             "camera_grad_maps=True carries it)")
        if mapping is not None and not cam_maps:
            raise ValueError("render: distortion together with a camera that requires grad is not supported: the map's "
                             "share of a pose gradient is out of scope (detach the camera; camera_grad_maps=True carries it)")
    if features is None and features_geom_grad and not normals:
        raise ValueError("render: features_geom_grad=True without features: pass the [P, C] tensor the map is blended from")
    if aux is None:   # nothing changes: no recorder, no extra launch, the same dictionary
        if aux_grad:
            raise ValueError("render: aux_grad=True without aux: name the maps the loss is put on")
        if features is None and not normals and mapping is None:
            return _render(*args, **kwargs)
        aux = ()
    aux = tuple(aux)
    for name in aux:
        if name not in _C.AUX_MAPS:
            raise ValueError(f"render: unknown aux map {name!r} (expected a subset of {_C.AUX_MAPS})")
    if aux_grad and not torch.is_grad_enabled():
        raise ValueError("render: aux_grad=True under no_grad: there is no graph to attach the maps to")
    camera = args[0] if args else kwargs["viewpoint_camera"]
    a = _SIGNATURE.bind(*args, **kwargs)
    a.apply_defaults()
    a = a.arguments
    pc, pipe = a["pc"], a["pipe"]
    if normals:                # (before anything is launched)
        _checked_normals(camera, pc, pipe, features)
        if features is None and features_geom_grad:
            _checked_geom_grad(pc, camera, cam_maps)
    if features is not None:   # (before anything is launched)
        _checked_features(features, pc, features_geom_grad, camera, cam_maps)
    # the distortion map is attached whenever there is a graph to attach it to; a QuantisedModel gets the detached map
    dist_attach = mapping is not None and torch.is_grad_enabled() and not isinstance(pc, QuantisedModel)
    if mapping is not None and isinstance(pc, QuantisedModel) and pc.trainable and torch.is_grad_enabled():
        raise ValueError("render: distortion for a trainable QuantisedModel is not supported (gradients of its codebooks "
                         "through the distortion map are out of scope); render it under no_grad for the detached map")
    user_channels = None if features is None else int(features.shape[1])
    if normals:   # the three channels ride the feature launch, behind the user's
        n = _model_normals(pc, pipe, _settings(camera, pc, pipe, a["bg_color"], a["scaling_modifier"]), a["override_color"],
                           a["variable_sh_bands"])
        features = n if features is None else torch.cat((features, n), dim=1)

    def blended(out):   # "features" as the launch left it -> the user's channels and the "normal" map
        if normals:
            both = out.pop("features")
            out["normal"] = both[user_channels or 0:]
            if user_channels is not None:
                out["features"] = both[:user_channels]
        return out
    if not aux_grad and not features_geom_grad and not dist_attach:
        with _C.forward_state() as st:
            out = _render(*args, **kwargs)
        out = _with_aux(aux, camera, out, st.result)
        if mapping is not None:
            out["distortion"] = _distortion_map(mapping, camera, out, st.result, None, None)
        if features is not None:
            out["features"] = _feature_map(features, camera, out, st.result,
                                           _settings(camera, pc, pipe, a["bg_color"], a["scaling_modifier"]))
        return blended(out)
    if aux_grad and isinstance(pc, QuantisedModel) and not pc.trainable:   # (before anything is launched)
        raise ValueError("render: aux_grad=True needs a trainable model (requires_grad_ the QuantisedModel first)")
    _tls.inputs = got = {}
    try:
        with _C.forward_state() as st:
            out = _render(*args, **kwargs)
    finally:
        _tls.inputs = None
    means3D, opacities, scales, rotations, cov3D = got["inputs"]
    trainable = any(t is not None and t.requires_grad for t in got["inputs"])
    if not trainable and (aux_grad or features_geom_grad) and not cam_maps:   # (a tracker: the camera alone is fitted)
        raise ValueError(f"render: {'aux_grad' if aux_grad else 'features_geom_grad'}=True for a model with nothing trainable")
    rs = _settings(camera, pc, pipe, a["bg_color"], a["scaling_modifier"])
    if mapping is not None:   # (nothing trainable: the detached map)
        out["distortion"] = _distortion_map(mapping, camera, out, st.result, rs, got["inputs"] if trainable or cam_maps else None,
                                            cam_maps)
    if features is not None:
        out["features"] = _feature_map(features, camera, out, st.result, rs, got["inputs"] if features_geom_grad else None,
                                       cam_maps and features_geom_grad)
    out = blended(out)
    if not aux_grad:
        return _with_aux(aux, camera, out, st.result)
    if st.result is None:   # an empty model: nothing was rendered -- zero maps, attached all the same
        out = _with_aux(aux, camera, out, None)
        out.update({name: _anchored(out[name], got["inputs"]) for name in aux})
        return out
    attached = aux_maps_with_camera_grad if cam_maps else aux_maps_with_grad
    out.update(attached(means3D, out["viewspace_points"], opacities, scales, rotations, cov3D, st.result, rs, maps=aux))
    return out
