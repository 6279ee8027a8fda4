"""`r3dgs_mip` -- anti-aliased rendering on the MI355X in HIP (csrc/mip.hip, csrc/mip_math.h, include/r3dgs_mip.h): the per-view
2D opacity compensation and the 3D smoothing filter, as differentiable maps from raw parameters to raw parameters that sit in
front of the unchanged rasterizer.  Every forward of this package applies sigmoid to the raw opacity it is given, so a
compensated opacity travels as its logit and autograd composes the maps with the rasterizer's own backward.

    from r3dgs_mip import filter_3d, pack_cameras
    from r3dgs_render import render

    cams = pack_cameras(train_cameras, device)            # once
    f = filter_3d(gaussians._xyz, cams)                   # after every densification, and every 100 iterations
    out = render(camera, gaussians, pipe, bg, antialiasing=True, filter_3d=f)

2D compensation (`antialias_opacity`, render(antialiasing=True)): with (a, b, c) the projected covariance BEFORE the forward's
0.3 dilation,  rho = sqrt(max(0.000025, (a c - b^2) / ((a + 0.3)(c + 0.3) - b^2))),  opacity_eff = sigmoid(o) rho.  These are the
`antialiasing` semantics of the official 3DGS rasterizer and gsplat's rasterize_mode="antialiased" with eps2d = 0.3.  They are
NOT Mip-Splatting's 2D filter, which replaces the dilation by a 0.1 kernel; the forward's dilation stays 0.3 here.

3D smoothing filter (`filter_3d`, `filtered_parameters`, render(filter_3d=f), `bake`): Mip-Splatting's.  filter_i =
d_i / max focal_x * sqrt(0.2), d_i the smallest view depth over the cameras that see Gaussian i (z > 0.2, projection within 15 %
of the image); scale_eff^2 = scale^2 + filter^2 and the opacity is multiplied by sqrt(prod scale^2 / prod scale_eff^2).

Nothing here waits on the host, allocates in the library or uses a float atomic; every call is capturable in a graph and
bit-identical from run to run.  Host tensors are refused (no CPU path), as are wrong dtypes and shapes.
"""
import math

import torch

from diff_gaussian_rasterization import _C

__all__ = ["antialias_opacity", "filter_3d", "pack_cameras", "filtered_parameters", "bake", "CAMERA_FLOATS"]

_lib = _C._lib   # the r3dgs_mip_* prototypes are rows of the required group of _C's ABI table
CAMERA_FLOATS = 20   # R3DGS_MIP_CAMERA_FLOATS: world_view_transform (16), focal_x, focal_y, W, H


def _ptr(t):
    return None if t is None else t.data_ptr()


def _input(what, name, t, shape, dev=None):
    """A float32 device tensor of the given shape, contiguous (copied if it is not) -- or a refusal."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {name} is {t.dtype}, expected torch.float32")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} is a host tensor; the anti-aliasing kernels need device tensors (no CPU path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: {name} is on {t.device}, expected {dev}")
    return t.contiguous()


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(status, what):
    if status < 0:
        raise RuntimeError(f"{what}: {_lib.r3dgs_last_error().decode()}")


class _AntialiasOpacity(torch.autograd.Function):
    """raw_eff [P,1] from (means3D, opacities, scales, rotations, cov3D_precomp) and one view (include/r3dgs_mip.h)."""

    @staticmethod
    def forward(ctx, means3D, opacities, scales, rotations, cov3D, viewmatrix, tanfovx, tanfovy, W, H, scale_modifier, raw):
        what = "antialias_opacity"
        P = means3D.shape[0] if isinstance(means3D, torch.Tensor) and means3D.dim() == 2 else -1
        means3D = _input(what, "means3D", means3D, (P, 3))
        dev = means3D.device
        opacities = _input(what, "opacities", opacities, (P, 1), dev)
        if cov3D is not None:
            if raw:
                raise ValueError(f"{what}: raw=True takes _scaling / _rotation, not cov3D_precomp")
            cov3D = _input(what, "cov3D_precomp", cov3D, (P, 6), dev)
            scales = rotations = None
        else:
            if scales is None or rotations is None:
                raise ValueError(f"{what}: provide a scale / rotation pair or cov3D_precomp")
            scales = _input(what, "scales", scales, (P, 3), dev)
            rotations = _aligned16(_input(what, "rotations", rotations, (P, 4), dev))
        viewmatrix = _input(what, "viewmatrix", viewmatrix, (4, 4), dev)
        raw_eff = torch.empty((P, 1), dtype=torch.float32, device=dev)
        ctx.view = (float(tanfovx), float(tanfovy), int(W), int(H), float(scale_modifier), int(bool(raw)))
        ctx.save_for_backward(means3D, opacities, scales, rotations, cov3D, viewmatrix)
        if P:
            with _C._on_device(dev):
                _check(_lib.r3dgs_mip_opacity(P, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3D), _ptr(opacities),
                                              ctx.view[5], _ptr(viewmatrix), ctx.view[0], ctx.view[1], ctx.view[2], ctx.view[3],
                                              ctx.view[4], _ptr(raw_eff), None, _C._stream()), what)
        return raw_eff

    @staticmethod
    def backward(ctx, g):
        means3D, opacities, scales, rotations, cov3D, viewmatrix = ctx.saved_tensors
        tanfovx, tanfovy, W, H, mod, raw = ctx.view
        P, dev = means3D.shape[0], means3D.device
        need = ctx.needs_input_grad
        new = lambda want, *shape: torch.empty(shape, dtype=torch.float32, device=dev) if want else None
        d_means, d_o = new(need[0], P, 3), new(need[1], P, 1)
        d_scales = new(need[2] and scales is not None, P, 3)
        d_rot = new(need[3] and rotations is not None, P, 4)
        d_cov = new(need[4] and cov3D is not None, P, 6)
        if P:
            g = g.contiguous()
            with _C._on_device(dev):
                _check(_lib.r3dgs_mip_opacity_backward(P, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3D), _ptr(opacities),
                                                       raw, _ptr(viewmatrix), tanfovx, tanfovy, W, H, mod, _ptr(g), _ptr(d_o),
                                                       _ptr(d_means), _ptr(d_scales), _ptr(d_rot), _ptr(d_cov), _C._stream()),
                       "antialias_opacity (backward)")
        return (d_means, d_o, d_scales, d_rot, d_cov) + (None,) * 7


def antialias_opacity(means3D, opacities, scales, rotations, cov3D_precomp, raster_settings, raw=False):
    """The per-view 2D compensation: raw opacities [P,1] -> raw_eff [P,1] with sigmoid(raw_eff) = sigmoid(o) rho, differentiable
    with respect to means3D, opacities and scales + rotations (or cov3D_precomp).  scales / rotations are activated values, or
    -- raw=True -- the model's _scaling / _rotation, activated by the kernel.  raster_settings: the
    GaussianRasterizationSettings of the view (image size, tan fov, viewmatrix, scale_modifier).  Hand the result to the
    rasterizer in place of the raw opacities; a Gaussian the forward culls (view z <= 0.2) keeps its opacity."""
    rs = raster_settings
    return _AntialiasOpacity.apply(means3D, opacities, scales, rotations, cov3D_precomp, rs.viewmatrix, rs.tanfovx, rs.tanfovy,
                                   rs.image_width, rs.image_height, rs.scale_modifier, raw)


def antialias_rho(means3D, opacities, scales, rotations, cov3D_precomp, raster_settings, raw=False):
    """-> (raw_eff [P,1], rho [P]) without a graph: the compensation factor itself, for inspection and tests."""
    rs, what = raster_settings, "antialias_rho"
    P = means3D.shape[0]
    means3D = _input(what, "means3D", means3D.detach(), (P, 3))
    dev = means3D.device
    opacities = _input(what, "opacities", opacities.detach(), (P, 1), dev)
    if cov3D_precomp is not None:
        cov3D_precomp, scales, rotations = _input(what, "cov3D_precomp", cov3D_precomp.detach(), (P, 6), dev), None, None
    else:
        scales = _input(what, "scales", scales.detach(), (P, 3), dev)
        rotations = _aligned16(_input(what, "rotations", rotations.detach(), (P, 4), dev))
    view = _input(what, "viewmatrix", rs.viewmatrix.detach(), (4, 4), dev)
    raw_eff = torch.empty((P, 1), dtype=torch.float32, device=dev)
    rho = torch.empty((P,), dtype=torch.float32, device=dev)
    if P:
        with _C._on_device(dev):
            _check(_lib.r3dgs_mip_opacity(P, _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3D_precomp), _ptr(opacities),
                                          int(bool(raw)), _ptr(view), float(rs.tanfovx), float(rs.tanfovy), int(rs.image_width),
                                          int(rs.image_height), float(rs.scale_modifier), _ptr(raw_eff), _ptr(rho), _C._stream()),
                   what)
    return raw_eff, rho


def pack_cameras(cameras, device=None):
    """The camera table of filter_3d: float32 [V, 20] on the device, a row per camera -- world_view_transform (16), focal_x,
    focal_y, W, H.  `cameras`: objects shaped like the reference's Camera (world_view_transform, FoVx, FoVy, image_width,
    image_height).  Pack once and keep the table: the training cameras do not change."""
    rows = []
    for cam in cameras:
        W, H = float(cam.image_width), float(cam.image_height)
        view = torch.as_tensor(cam.world_view_transform, dtype=torch.float32).detach().reshape(16).cpu()
        rows.append(torch.cat([view, torch.tensor([W / (2.0 * math.tan(cam.FoVx * 0.5)), H / (2.0 * math.tan(cam.FoVy * 0.5)), W, H],
                                                  dtype=torch.float32)]))
    table = torch.stack(rows) if rows else torch.zeros((0, CAMERA_FLOATS), dtype=torch.float32)
    return table.to(device) if device is not None else table


def filter_3d(xyz, cameras, out=None, workspace=None):
    """Mip-Splatting's 3D filter: float32 [P,1] from the positions and a camera set, in two launches without a host wait.
    cameras: the table pack_cameras made (float32 [V,20] on xyz's device) -- or a list of camera objects, packed here (pack it
    once yourself if you call this more than once).  out / workspace: optional preallocated result and scratch
    (uint8, at least workspace_bytes(P, V)), for a capture in a graph."""
    what = "filter_3d"
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2:
        raise TypeError(f"{what}: xyz must be a [P,3] tensor")
    P = xyz.shape[0]
    xyz = _input(what, "xyz", xyz.detach(), (P, 3))
    dev = xyz.device
    if not isinstance(cameras, torch.Tensor):
        cameras = pack_cameras(cameras, dev)
    V = cameras.shape[0] if cameras.dim() == 2 else -1
    cameras = _input(what, "cameras", cameras, (V, CAMERA_FLOATS), dev)
    if out is None:
        out = torch.empty((P, 1), dtype=torch.float32, device=dev)
    else:
        out = _input(what, "out", out, (P, 1), dev)
    if P == 0:
        return out
    nbytes = int(_lib.r3dgs_mip_filter3d_workspace_bytes(P, V))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or workspace.numel() < nbytes or workspace.data_ptr() % 16:
        raise ValueError(f"{what}: workspace must be a 16-byte aligned uint8 tensor of at least {nbytes} bytes on {dev}")
    with _C._on_device(dev):
        _check(_lib.r3dgs_mip_filter3d(P, V, _ptr(xyz), _ptr(cameras) if V else None, _ptr(out), _ptr(workspace), _C._stream()), what)
    return out


def workspace_bytes(P, V):
    return int(_lib.r3dgs_mip_filter3d_workspace_bytes(int(P), int(V)))


class _Filtered(torch.autograd.Function):
    """(scaling_eff [P,3], opacity_eff [P,1]) from (scaling_raw, opacity_raw, filter): one fused kernel each way."""

    @staticmethod
    def forward(ctx, scaling_raw, opacity_raw, filt):
        what = "filtered_parameters"
        P = scaling_raw.shape[0] if isinstance(scaling_raw, torch.Tensor) and scaling_raw.dim() == 2 else -1
        scaling_raw = _input(what, "scaling_raw", scaling_raw, (P, 3))
        dev = scaling_raw.device
        opacity_raw = _input(what, "opacity_raw", opacity_raw, (P, 1), dev)
        filt = _input(what, "filter_3d", filt, (P, 1), dev)
        scaling_eff, opacity_eff = torch.empty_like(scaling_raw), torch.empty_like(opacity_raw)
        ctx.save_for_backward(scaling_raw, opacity_raw, filt)
        if P:
            with _C._on_device(dev):
                _check(_lib.r3dgs_mip_filtered(P, _ptr(scaling_raw), _ptr(opacity_raw), _ptr(filt), _ptr(scaling_eff),
                                               _ptr(opacity_eff), _C._stream()), what)
        return scaling_eff, opacity_eff

    @staticmethod
    def backward(ctx, g_scaling, g_opacity):
        scaling_raw, opacity_raw, filt = ctx.saved_tensors
        P, dev = scaling_raw.shape[0], scaling_raw.device
        d_scaling = torch.empty_like(scaling_raw) if ctx.needs_input_grad[0] else None
        d_opacity = torch.empty_like(opacity_raw) if ctx.needs_input_grad[1] else None
        if P:
            g_scaling = None if g_scaling is None else g_scaling.contiguous()
            g_opacity = None if g_opacity is None else g_opacity.contiguous()
            with _C._on_device(dev):
                _check(_lib.r3dgs_mip_filtered_backward(P, _ptr(scaling_raw), _ptr(opacity_raw), _ptr(filt), _ptr(g_scaling),
                                                        _ptr(g_opacity), _ptr(d_scaling), _ptr(d_opacity), _C._stream()),
                       "filtered_parameters (backward)")
        return d_scaling, d_opacity, None


def filtered_parameters(scaling_raw, opacity_raw, filter_3d):
    """The 3D filter applied to the model's raw _scaling [P,3] and _opacity [P,1] -> (log_scale_eff, raw_opacity_eff), raw
    parameters again: exp(log_scale_eff)^2 = exp(scaling_raw)^2 + filter^2 and sigmoid(raw_opacity_eff) = sigmoid(opacity_raw)
    sqrt(prod s^2 / prod s_eff^2).  Differentiable in the two parameters; filter_3d [P,1] carries no gradient.  Rows with
    filter == 0 are the inputs, bit for bit."""
    return _Filtered.apply(scaling_raw, opacity_raw, filter_3d)


def bake(pc, filter_3d):
    """Writes the filtered values into pc._scaling / pc._opacity (under no_grad), for export to a viewer that knows nothing of
    the filter: the forward op and an assignment."""
    with torch.no_grad():
        scaling, opacity = filtered_parameters(pc._scaling.detach(), pc._opacity.detach(), filter_3d)
        for name, new in (("_scaling", scaling), ("_opacity", opacity)):
            old = getattr(pc, name)
            if isinstance(old, torch.nn.Parameter):
                old.data = new
            else:
                setattr(pc, name, new)
    return pc
