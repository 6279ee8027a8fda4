"""`r3dgs_normals` -- surface normals on the MI355X in HIP (csrc/normals.hip, csrc/normal_math.h, include/r3dgs_normals.h): the
view-space normal of every Gaussian, the normal map derived from a depth map by finite differences, and the depth-normal
consistency loss every surface-aligned splatting method trains with (2DGS, GOF, PGSR, RaDe-GS), each with its backward.

    from r3dgs_render import render
    import r3dgs_normals

    out = render(view, gaussians, pipe, bg, aux=("depth", "alpha"), aux_grad=True, normals=True, features_geom_grad=True)
    Ln, surf = r3dgs_normals.normal_consistency(out["normal"], out["depth"], rs_of(view), alpha=out["alpha"])
    loss = image_loss + lambda_normal * Ln

Normal of a Gaussian (`gaussian_normals`, render(normals=True)): the axis of its smallest scale (lowest index on a tie) --
column k of the rotation R of Sigma = R S^2 R^T -- turned towards the camera (negated when n . (mean - campos) > 0) and taken
into the view frame.  The gradient reaches the rotations alone; scales and means receive None.

Normal of a depth pixel (`depth_to_normal`): z = depth / alpha where alpha >= ALPHA_MIN (else 0; no alpha: z = depth), points
un-projected through the pixel centres, n = normalize(d_v x d_h) from central differences; 0 where |d_v x d_h|^2 <= CROSS_MIN
and on the one-pixel border.  View frame: a fronto-parallel plane gives (0, 0, -1), facing the camera like the Gaussians'.

Loss (`normal_consistency`): mean over ALL pixels of w (1 - s N . n), N the blended, unnormalised "normal" map, s = alpha
detached (scale_by_alpha) or 1, w an optional [H,W] weight (0 leaves a pixel out of the sum, not out of the divisor).

Nothing here waits on the host, allocates in the library or uses a float atomic; the loss and its upstream gradient stay on the
device; every call is capturable in a graph and bit-identical from run to run.  Wrong shapes, dtypes and devices are refused
with a ValueError (there is no CPU path).  The calls go through ctypes; the compiled torch binding does not carry them.
"""
import torch

from diff_gaussian_rasterization import _C

__all__ = ["gaussian_normals", "depth_to_normal", "normal_consistency", "ALPHA_MIN", "CROSS_MIN"]

_lib = _C._lib   # the prototypes of include/r3dgs_normals.h are rows of the required group of _C's ABI table
ALPHA_MIN = 1e-3    # R3DGS_NORMAL_ALPHA_MIN
CROSS_MIN = 1e-24   # R3DGS_NORMAL_CROSS_MIN


def _ptr(t):
    return None if t is None else t.data_ptr()


def _input(what, name, t, shape, dev=None):
    """A float32 device tensor of the given shape, contiguous (copied if it is not) -- or a ValueError."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} is {t.dtype}, expected torch.float32")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_cuda:
        raise ValueError(f"{what}: {name} is a host tensor; the normal kernels need device tensors (no CPU path)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: {name} is on {t.device}, expected {dev} (the model's device)")
    return t.contiguous()


def _aligned16(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(status, what):
    if status < 0:
        raise RuntimeError(f"{what}: {_lib.r3dgs_last_error().decode()}")


class _GaussianNormals(torch.autograd.Function):
    """normals [P,3] from (means3D, scales, rotations) and one view: one launch each way (include/r3dgs_normals.h)."""

    @staticmethod
    def forward(ctx, means3D, scales, rotations, viewmatrix, campos, raw):
        what = "gaussian_normals"
        if scales is None or rotations is None:
            raise ValueError(f"{what}: needs scales and rotations; a precomputed covariance (cov3D_precomp) has no axis to pick")
        P = means3D.shape[0] if isinstance(means3D, torch.Tensor) and means3D.dim() == 2 else -1
        means3D = _input(what, "means3D", means3D, (P, 3))
        dev = means3D.device
        scales = _input(what, "scales", scales, (P, 3), dev)
        rotations = _aligned16(_input(what, "rotations", rotations, (P, 4), dev))
        viewmatrix = _input(what, "viewmatrix", viewmatrix, (4, 4), dev)
        campos = _input(what, "campos", campos, (3,), dev)
        normals = torch.empty((P, 3), dtype=torch.float32, device=dev)
        ctx.raw = int(bool(raw))
        ctx.save_for_backward(means3D, scales, rotations, viewmatrix, campos)
        if P:
            with _C._on_device(dev):
                _check(_lib.r3dgs_gaussian_normals(P, _ptr(means3D), _ptr(scales), _ptr(rotations), ctx.raw, _ptr(viewmatrix),
                                                   _ptr(campos), _ptr(normals), _C._stream()), what)
        return normals

    @staticmethod
    def backward(ctx, g):
        means3D, scales, rotations, viewmatrix, campos = ctx.saved_tensors
        P, dev = means3D.shape[0], means3D.device
        d_rot = None
        if ctx.needs_input_grad[2]:
            d_rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
            if P:
                g = g.contiguous()
                with _C._on_device(dev):
                    _check(_lib.r3dgs_gaussian_normals_backward(P, _ptr(means3D), _ptr(scales), _ptr(rotations), ctx.raw,
                                                                _ptr(viewmatrix), _ptr(campos), _ptr(g), _ptr(d_rot), _C._stream()),
                           "gaussian_normals (backward)")
        return None, None, d_rot, None, None, None   # the argmin and the sign are piecewise constant


def gaussian_normals(means3D, scales, rotations, raster_settings, raw=False):
    """The view-space normal of every Gaussian -> float32 [P,3], differentiable with respect to `rotations`.  scales / rotations
    are activated values (the rotations unit quaternions, used as given) or -- raw=True -- the model's _scaling / _rotation, the
    quaternion normalised by the kernel.  raster_settings: the GaussianRasterizationSettings of the view (viewmatrix, campos)."""
    rs = raster_settings
    return _GaussianNormals.apply(means3D, scales, rotations, rs.viewmatrix, rs.campos, raw)


def _image(what, depth, alpha, normal_map, pixel_weight):
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.shape[0] != 1:
        shape = tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth).__name__
        raise ValueError(f"{what}: depth must be a [1,H,W] tensor, got {shape}")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    depth = _input(what, "depth", depth, (1, H, W))
    dev = depth.device
    if alpha is not None:
        alpha = _input(what, "alpha", alpha, (1, H, W), dev)
    if normal_map is not None:
        normal_map = _input(what, "normal_map", normal_map, (3, H, W), dev)
    if pixel_weight is not None:
        pixel_weight = _input(what, "pixel_weight", pixel_weight, (H, W), dev)
    return H, W, dev, depth, alpha, normal_map, pixel_weight


class _DepthNormal(torch.autograd.Function):
    """(surf_normal [3,H,W], loss) from (depth, alpha, normal_map); normal_map None: the normals alone (loss is None)."""

    @staticmethod
    def forward(ctx, depth, alpha, normal_map, pixel_weight, tanfovx, tanfovy, scale_by_alpha, what):
        H, W, dev, depth, alpha, normal_map, pixel_weight = _image(what, depth, alpha, normal_map, pixel_weight)
        surf = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        loss = ws = None
        if normal_map is not None:
            loss = torch.zeros((), dtype=torch.float32, device=dev)
            ws = torch.empty(max(8, int(_lib.r3dgs_depth_normal_workspace_bytes(H, W))), dtype=torch.uint8, device=dev)
        ctx.view = (H, W, float(tanfovx), float(tanfovy), int(bool(scale_by_alpha)), what)
        ctx.save_for_backward(depth, alpha, normal_map, pixel_weight)
        if H and W:
            with _C._on_device(dev):
                _check(_lib.r3dgs_depth_normal(H, W, ctx.view[2], ctx.view[3], _ptr(depth), _ptr(alpha), _ptr(normal_map),
                                               _ptr(pixel_weight), ctx.view[4], _ptr(surf), _ptr(loss), _ptr(ws), _C._stream()), what)
        if normal_map is None:
            return surf
        ctx.mark_non_differentiable(surf)
        return loss, surf

    @staticmethod
    def backward(ctx, *gs):
        depth, alpha, normal_map, pixel_weight = ctx.saved_tensors
        H, W, tanfovx, tanfovy, scale_by_alpha, what = ctx.view
        dev, need = depth.device, ctx.needs_input_grad
        g_loss, g_surf = (gs[0], None) if normal_map is not None else (None, gs[0])
        run = bool(H and W and (g_loss is not None or g_surf is not None))   # the kernel writes every element of every output
        new = lambda want, c: (torch.empty if run else torch.zeros)((c, H, W), dtype=torch.float32, device=dev) if want else None
        d_depth, d_alpha, d_normal = new(need[0], 1), new(need[1] and alpha is not None, 1), new(need[2] and normal_map is not None, 3)
        if run:
            g_loss = None if g_loss is None else g_loss.contiguous()
            g_surf = None if g_surf is None else g_surf.contiguous()
            with _C._on_device(dev):
                _check(_lib.r3dgs_depth_normal_backward(H, W, tanfovx, tanfovy, _ptr(depth), _ptr(alpha), _ptr(normal_map),
                                                        _ptr(pixel_weight), scale_by_alpha, _ptr(g_loss), _ptr(g_surf),
                                                        _ptr(d_depth), _ptr(d_alpha), _ptr(d_normal), _C._stream()),
                       what + " (backward)")
        return d_depth, d_alpha, d_normal, None, None, None, None, None


def depth_to_normal(depth, raster_settings, alpha=None):
    """The normal map of a [1,H,W] view-depth map -> float32 [3,H,W] in the view frame, differentiable with respect to `depth`
    and -- through z = depth / alpha -- `alpha` ([1,H,W]; pass it with the project's unnormalised "depth", leave it out with
    "median_depth").  raster_settings: tanfovx, tanfovy of the view."""
    rs = raster_settings
    return _DepthNormal.apply(depth, alpha, None, None, rs.tanfovx, rs.tanfovy, False, "depth_to_normal")


def normal_consistency(normal_map, depth, raster_settings, alpha=None, scale_by_alpha=True, pixel_weight=None):
    """The depth-normal consistency loss -> (loss: float32 0-dim tensor on the device, surf_normal: float32 [3,H,W], detached).
    normal_map: the blended, unnormalised [3,H,W] map (render(normals=True)["normal"]); depth / alpha: as `depth_to_normal`;
    scale_by_alpha: multiply the depth normal by alpha as a constant (2DGS's rend_alpha.detach()); pixel_weight: optional [H,W]
    weights.  Gradients reach normal_map, depth and, through the division only, alpha."""
    if normal_map is None:
        raise ValueError("normal_consistency: normal_map is None (depth_to_normal gives the normals alone)")
    rs = raster_settings
    return _DepthNormal.apply(depth, alpha, normal_map, pixel_weight, rs.tanfovx, rs.tanfovy, scale_by_alpha, "normal_consistency")
