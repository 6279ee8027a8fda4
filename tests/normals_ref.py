"""float64 torch restatement of the surface-normal unit (include/r3dgs_normals.h) for tests/test_normals_cpu.py and
tests/test_normals_gpu.py, differentiated by autograd, evaluated from the same fp32 inputs as the kernels and written without
looking at csrc/normal_math.h: the axis is a column of the reference's build_rotation matrix, the depth normal is 2DGS's
depth_to_normal as published (un-project every pixel, subtract the un-projected points, cross, normalize), kept in the view
frame.

The operators take DECISIONS -- which scale is the smallest, which way the axis faces, whether alpha is large enough to divide
by, whether the cross product has a direction.  The seeded inputs of `gaussians` and `image` keep a margin from every one of
them and `check_margins_*` asserts it, so the tests compare every element and mask none."""
import numpy as np
import torch

F32 = np.float32
DT = torch.float64
ALPHA_MIN, CROSS_MIN = 1e-3, 1e-24   # the header's constants
SCALE_GAP = 1e-3      # relative gap between the two smallest scales
FACING_FLOOR = 1e-3   # |n_w . (mean - campos)| / |mean - campos|
CROSS_MARGIN = 1e6    # |c|^2 is this factor above CROSS_MIN, or c is exactly zero
ALPHA_MARGIN = 2.0    # alpha is this factor above ALPHA_MIN, or exactly zero


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def build_rotation(q):
    """The reference's utils.general_utils.build_rotation without its normalisation: R of a quaternion (r, x, y, z) [P,4]."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1)
    return R.reshape(-1, 3, 3)


def gaussian_normals(means3D, scales, rotations, viewmatrix, campos, raw=False, parts=False):
    """float64 tensors -> [P,3].  raw: rotations are divided by max(|q|, 1e-12) (F.normalize); scales are only compared."""
    q = rotations / rotations.norm(dim=1, keepdim=True).clamp_min(1e-12) if raw else rotations
    R = build_rotation(q)
    k = torch.argmin(scales.detach(), dim=1)   # torch.argmin returns the first of equal minima
    n_w = torch.gather(R, 2, k.reshape(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)
    facing = (n_w.detach() * (means3D - campos)).sum(1)
    n_w = torch.where((facing > 0)[:, None], -n_w, n_w)
    out = n_w @ viewmatrix[:3, :3]
    return (out, k, facing) if parts else out


def pixel_z(depth, alpha):
    if alpha is None:
        return depth
    live = alpha.detach() >= ALPHA_MIN
    return torch.where(live, depth / torch.where(live, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))


def depth_to_normal(depth, alpha, tanfovx, tanfovy, parts=False):
    """depth, alpha: float64 [H,W] -> [3,H,W].  2DGS: points = z * ray of the pixel centre; dx = points[2:, 1:-1] -
    points[:-2, 1:-1]; dy = points[1:-1, 2:] - points[1:-1, :-2]; normalize(cross(dx, dy)); zero border."""
    H, W = depth.shape
    z = pixel_z(depth, alpha)
    xs = (2.0 * (torch.arange(W, dtype=DT) + 0.5) / W - 1.0) * tanfovx
    ys = (2.0 * (torch.arange(H, dtype=DT) + 0.5) / H - 1.0) * tanfovy
    rays = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), torch.ones(H, W, dtype=DT)], dim=-1)
    points = z[..., None] * rays
    out = torch.zeros(H, W, 3, dtype=DT)
    c2 = torch.zeros(H, W, dtype=DT)
    if H >= 3 and W >= 3:
        dx = points[2:, 1:-1] - points[:-2, 1:-1]
        dy = points[1:-1, 2:] - points[1:-1, :-2]
        c = torch.cross(dx, dy, dim=-1)
        len2 = (c * c).sum(-1)
        live = len2.detach() > CROSS_MIN
        n = torch.where(live[..., None], c / torch.where(live, len2, torch.ones_like(len2)).sqrt()[..., None], torch.zeros_like(c))
        out = torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
        c2 = torch.nn.functional.pad(len2.detach(), (1, 1, 1, 1))
    out = out.permute(2, 0, 1)
    return (out, c2) if parts else out


def normal_consistency(normal_map, depth, alpha, tanfovx, tanfovy, scale_by_alpha=True, pixel_weight=None):
    """-> (loss, surf_normal [3,H,W]) in float64."""
    n = depth_to_normal(depth, alpha, tanfovx, tanfovy)
    s = alpha.detach() if (scale_by_alpha and alpha is not None) else torch.ones_like(depth)
    w = pixel_weight if pixel_weight is not None else torch.ones_like(depth)
    return (w * (1.0 - s * (normal_map * n).sum(0))).sum() / depth.numel(), n


# ---- seeded inputs with their margins ------------------------------------------------------------------------------------------

TAN_FOVX, TAN_FOVY = 0.62, 0.41


def view_of(seed=0):
    """-> (viewmatrix [4,4] fp32, row-vector convention, campos [3] fp32): a rotated, translated camera."""
    rng = np.random.default_rng(100 + seed)
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    c = rng.uniform(-1, 1, 3)
    V = np.eye(4)
    V[:3, :3] = Q          # p_view = p_world Q + t
    V[3, :3] = -c @ Q
    return V.astype(F32), c.astype(F32)


def gaussians(P, seed):
    """-> dict of fp32 arrays: means3D, scales, scaling_raw, rotations (unit), rotation_raw, with the argmin spread over the
    three axes and the margins of check_margins_gaussians."""
    rng = np.random.default_rng(seed)
    V, c = view_of(seed)
    means = (c + rng.normal(0, 3, (P, 3))).astype(F32)
    base = np.exp(rng.normal(-3, 1, (P, 1)))
    mult = 1.0 + rng.uniform(0.05, 4.0, (P, 3))
    mult[np.arange(P), rng.integers(0, 3, P)] = 1.0
    scales = (base * mult).astype(F32)
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rot = q.astype(F32)
    rot_raw = (q * 10.0 ** rng.uniform(-1, 1, (P, 1))).astype(F32)
    g = dict(means3D=means, scales=scales, scaling_raw=np.log(scales).astype(F32), rotations=rot, rotation_raw=rot_raw,
             viewmatrix=V, campos=c)
    return with_facing_margin(g)


def check_margins_gaussians(g, raw, scale_gap=SCALE_GAP, facing_floor=FACING_FLOOR):
    """Asserts the margins of one case -> (k, facing).  The seeded cases keep the defaults.  A scene that was not built for this
    test passes scale_gap=0 and a small facing_floor, which is still safe: the kernel and the reference compare the SAME fp32
    scales (equal ones go to the lowest index in both), and both evaluate the facing dot product in double from the same fp32
    inputs, so the two differ by ~1e-15 of |mean - campos| and a floor of 1e-9 keeps six digits of margin."""
    s = np.sort(g["scaling_raw" if raw else "scales"].astype(np.float64), axis=1)
    lin = np.exp(s) if raw else s
    assert ((lin[:, 1] - lin[:, 0]) >= scale_gap * lin[:, 1]).all(), "two smallest scales too close"
    _, k, facing = gaussian_normals(_t(g["means3D"]), _t(g["scaling_raw" if raw else "scales"]),
                                    _t(g["rotation_raw" if raw else "rotations"]), _t(g["viewmatrix"]), _t(g["campos"]), raw=raw,
                                    parts=True)
    d = np.linalg.norm(g["means3D"].astype(np.float64) - g["campos"], axis=1)
    assert (np.abs(facing.numpy()) >= facing_floor * d).all(), "a Gaussian is seen edge-on"
    return k.numpy(), facing.numpy()


def with_facing_margin(g):
    """The case with every Gaussian that is seen nearly edge-on (either quaternion form) pushed along its axis."""
    g = dict(g)
    m = g["means3D"].astype(np.float64)
    for _ in range(4):
        for key, raw in (("rotations", False), ("rotation_raw", True)):
            q = _t(g[key])
            qn = q / q.norm(dim=1, keepdim=True) if raw else q
            R = build_rotation(qn).numpy()
            k = np.argmin(g["scales"], axis=1)
            axis = R[np.arange(len(k)), :, k]
            d = m - g["campos"]
            f = (axis * d).sum(1)
            bad = np.abs(f) < 4 * FACING_FLOOR * np.linalg.norm(d, axis=1)
            m[bad] += axis[bad] * np.where(f[bad] >= 0, 1.0, -1.0)[:, None] * 0.5
    g["means3D"] = m.astype(F32)
    return g


def image(H, W, seed, with_holes=True):
    """-> dict of fp32 arrays for one image: depth [H,W] (UNNORMALISED: z * alpha), alpha [H,W], z_only [H,W] (a depth map to use
    without alpha), normal_map [3,H,W], weight [H,W], g_surf [3,H,W].  A smooth, tilted, wavy surface; alpha in [0.3, 1] with a
    hole of exact zeros (depth 0 too) when the image is large enough."""
    rng = np.random.default_rng(1000 + seed)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = xs / max(W - 1, 1), ys / max(H - 1, 1)
    z = 3.0 + 0.8 * u - 0.5 * v + 0.15 * np.sin(5.0 * u + 1.0) * np.cos(4.0 * v) + rng.uniform(-0.01, 0.01, (H, W))
    alpha = 0.3 + 0.7 * rng.uniform(0, 1, (H, W))
    if with_holes and H >= 16 and W >= 16:
        alpha[H // 3:H // 3 + 5, W // 2:W // 2 + 6] = 0.0
    alpha = alpha.astype(F32)
    depth = (z.astype(F32) * alpha).astype(F32)
    n = rng.normal(size=(3, H, W))
    n[2] -= 2.0
    n = n / np.linalg.norm(n, axis=0, keepdims=True) * alpha
    weight = rng.uniform(0.0, 2.0, (H, W))
    weight[rng.uniform(size=(H, W)) < 0.2] = 0.0
    return dict(depth=depth, alpha=alpha, z_only=z.astype(F32), normal_map=n.astype(F32), weight=weight.astype(F32),
                g_surf=rng.normal(size=(3, H, W)).astype(F32))


def check_margins_image(depth, alpha, tanfovx=TAN_FOVX, tanfovy=TAN_FOVY):
    """Asserts that alpha and |c|^2 keep away from their constants or sit exactly on the zero side -> |c|^2 [H,W]."""
    if alpha is not None:
        assert ((alpha == 0) | (alpha >= ALPHA_MARGIN * ALPHA_MIN)).all(), "alpha near R3DGS_NORMAL_ALPHA_MIN"
    _, c2 = depth_to_normal(_t(depth), _t(alpha), tanfovx, tanfovy, parts=True)
    c2 = c2.numpy()
    assert ((c2 == 0) | (c2 >= CROSS_MARGIN * CROSS_MIN)).all(), "|c|^2 near R3DGS_NORMAL_CROSS_MIN"
    return c2


def vjp(outputs, cotangents, leaves):
    leaves_ = [x for x in leaves if x is not None]
    total = sum((o * _t(np.asarray(c)).reshape(o.shape)).sum() if not isinstance(c, torch.Tensor) else (o * c).sum()
                for o, c in zip(outputs, cotangents))
    got = iter(torch.autograd.grad(total, leaves_, allow_unused=True))
    return [None if x is None else (lambda g, like: torch.zeros_like(like) if g is None else g)(next(got), x) for x in leaves]
