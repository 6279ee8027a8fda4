"""Float64 torch restatement of the anti-aliasing unit (include/r3dgs_mip.h), written from the formulas, with gradients by
autograd.  It shares no code with csrc/mip_math.h: the kernels derive their backward by hand, this file lets autograd do it.

    opacity(...)      the per-view 2D compensation:  rho = sqrt(max(0.000025, det C / det(C + 0.3 I))),  raw_eff = logit(sigmoid(o) rho)
    filter3d(...)     the 3D filter of a camera set:  d_i / max focal_x * sqrt(0.2)
    filtered(...)     the 3D filter applied:  ls_eff = 0.5 log(exp(2 ls) + f^2),  raw_eff = logit(sigmoid(o) coef)

Inputs are the fp32 numbers the kernels read, promoted to float64; the constants the forward forms in fp32 (focal lengths,
the 1.3 tan(fov) clamp limits) are formed in fp32 here too.  Each function also says which rows are AMBIGUOUS -- rows whose
decision a last-bit difference could flip -- so that a comparison can leave them out:
    opacity    view z within 1e-5 (relative) of 0.2;  the determinant ratio within 1e-4 (relative) of the 0.000025 floor
    filter3d   for any camera: z within 1e-5 (relative) of 0.2, or a projection within 1e-5 (relative) of a screen bound
A test may leave out at most 1 % of its rows (MAX_AMBIGUOUS).

The 1 - p floor of the logit (2^-24) is only reached for raw opacities above 16.6; there the kernels follow the cancelled
form (1 - s) / max(1 - p, 2^-24) literally, and this file's clamp passes no gradient.  The tests stay within +-15.
"""
import numpy as np
import torch

F64 = torch.float64
DILATION = 0.3
RATIO_FLOOR = 0.000025
ONE_MINUS_P_FLOOR = 2.0 ** -24
NEAR = float(np.float32(0.2))
MARGIN = float(np.float32(0.15))
FILTER_VAR = 0.2
MAX_AMBIGUOUS = 0.01


def _t(x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().to("cpu", F64)
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def view_constants(tan_fovx, tan_fovy, W, H):
    """The fp32 numbers the forward forms: focal lengths (W / (2 tan)) and the clamp limits (1.3 tan)."""
    tx, ty = np.float32(tan_fovx), np.float32(tan_fovy)
    return {"fx": float(np.float32(W) / (np.float32(2.0) * tx)), "fy": float(np.float32(H) / (np.float32(2.0) * ty)),
            "limx": float(np.float32(1.3) * tx), "limy": float(np.float32(1.3) * ty)}


def rotation_matrix(q):
    """R of a quaternion (r, x, y, z) as it is, NOT normalised (the forward's formula)."""
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def cov3d(scales, rotations, scale_modifier):
    M = rotation_matrix(rotations) * (scale_modifier * scales)[:, None, :]   # column k scaled by s_k
    return M @ M.transpose(1, 2)


def cov3d_from6(c6):
    i = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    return c6[:, i]


def activate(scaling_raw, rotation_raw):
    """exp and F.normalize (eps 1e-12), the model's activations."""
    n = rotation_raw.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.exp(scaling_raw), rotation_raw / n


def cov2d(means3D, Sigma, viewmatrix, k):
    """-> (a, b, c, z): the 2D covariance before the dilation and the view depth.  viewmatrix: [4,4] as the renderer passes it
    (world_view_transform: a point is a row vector on its left)."""
    V = viewmatrix.reshape(4, 4)
    t = means3D @ V[:3, :3] + V[3, :3]
    z = t[:, 2]
    zs = torch.where(z > NEAR, z, torch.ones_like(z))   # culled rows: any finite number (their result is replaced)
    tx = torch.clamp(t[:, 0] / zs, -k["limx"], k["limx"]) * zs
    ty = torch.clamp(t[:, 1] / zs, -k["limy"], k["limy"]) * zs
    zero = torch.zeros_like(zs)
    J = torch.stack([k["fx"] / zs, zero, -k["fx"] * tx / (zs * zs), zero, k["fy"] / zs, -k["fy"] * ty / (zs * zs)], -1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    C = A @ Sigma @ A.transpose(1, 2)
    return C[:, 0, 0], C[:, 0, 1], C[:, 1, 1], z


def logit_of_product(o, m):
    """logit(sigmoid(o) m), 1 - p floored at 2^-24."""
    p = torch.sigmoid(o) * m
    return torch.log(p) - torch.log(torch.clamp(1 - p, min=ONE_MINUS_P_FLOOR))


def opacity(means3D, opacities, scales, rotations, cov3D_precomp, viewmatrix, tan_fovx, tan_fovy, W, H, scale_modifier=1.0,
            raw=False):
    """-> (raw_eff [P,1], rho [P], ambiguous [P] bool).  Tensors that require grad (float64 leaves) stay attached."""
    k = view_constants(tan_fovx, tan_fovy, W, H)
    if cov3D_precomp is not None:
        Sigma = cov3d_from6(cov3D_precomp)
    else:
        s, q = activate(scales, rotations) if raw else (scales, rotations)
        Sigma = cov3d(s, q, float(np.float32(scale_modifier)))
    a, b, c, z = cov2d(means3D, Sigma, viewmatrix, k)
    det = a * c - b * b
    det_d = (a + DILATION) * (c + DILATION) - b * b
    ratio = det / det_d
    rho = torch.sqrt(torch.where(ratio > RATIO_FLOOR, ratio, torch.full_like(ratio, RATIO_FLOOR)))
    culled = ~(z > NEAR)
    rho = torch.where(culled, torch.ones_like(rho), rho)
    o = opacities.reshape(-1)
    raw_eff = torch.where(culled, o, logit_of_product(o, rho))
    amb = ((z - NEAR).abs() <= 1e-5 * NEAR) | (~culled & ((ratio - RATIO_FLOOR).abs() <= 1e-4 * RATIO_FLOOR))
    return raw_eff.reshape(-1, 1), rho, amb.detach()


def filter3d(xyz, cameras):
    """cameras: [V,20] rows (world_view_transform 16, focal_x, focal_y, W, H) -> (filter [P,1], ambiguous [P] bool)."""
    xyz, cameras = _t(xyz), _t(cameras).reshape(-1, 20)
    P = xyz.shape[0]
    d = torch.full((P,), float("inf"), dtype=F64)
    valid_any = torch.zeros(P, dtype=torch.bool)
    amb = torch.zeros(P, dtype=torch.bool)
    for cam in cameras:
        V, fx, fy, W, H = cam[:16].reshape(4, 4), cam[16], cam[17], cam[18], cam[19]
        t = xyz @ V[:3, :3] + V[3, :3]
        z = t[:, 2]
        zs = torch.where(z > NEAR, z, torch.ones_like(z))
        px, py = t[:, 0] / zs * fx + W / 2, t[:, 1] / zs * fy + H / 2
        ok = (z > NEAR) & (px >= -MARGIN * W) & (px <= (1 + MARGIN) * W) & (py >= -MARGIN * H) & (py <= (1 + MARGIN) * H)
        near = (z - NEAR).abs() <= 1e-5 * NEAR
        for pix, S in ((px, W), (py, H)):
            for thr in (-MARGIN * S, (1 + MARGIN) * S):
                near |= (z > NEAR) & ((pix - thr).abs() <= 1e-5 * thr.abs())
        amb |= near
        d = torch.where(ok, torch.minimum(d, z), d)
        valid_any |= ok
    dmax = d[valid_any].max() if bool(valid_any.any()) else torch.tensor(0.0, dtype=F64)
    d = torch.where(valid_any, d, dmax)
    focal = cameras[:, 16].max() if len(cameras) else torch.tensor(1.0, dtype=F64)
    return (d / focal * FILTER_VAR ** 0.5).reshape(-1, 1), amb


def filtered(scaling_raw, opacity_raw, filter_3d):
    """-> (log_scale_eff [P,3], raw_eff [P,1]); rows with f == 0 are the inputs themselves."""
    f2 = filter_3d.detach().reshape(-1, 1) ** 2
    s2 = torch.exp(2 * scaling_raw)
    ls_eff = 0.5 * torch.log(s2 + f2)
    coef = torch.sqrt((s2 / (s2 + f2)).prod(dim=1))
    raw_eff = logit_of_product(opacity_raw.reshape(-1), coef).reshape(-1, 1)
    zero = f2 == 0
    return torch.where(zero, scaling_raw, ls_eff), torch.where(zero, opacity_raw.reshape(-1, 1), raw_eff)


def leaves(*arrays):
    """float64 leaves that require grad, from fp32 arrays / tensors (None stays None)."""
    return [None if a is None else _t(a).requires_grad_() for a in arrays]


def vjp(outputs, cotangents, inputs):
    """The vector-Jacobian product: gradients of sum(outputs . cotangents) w.r.t. inputs (zeros for an unused one)."""
    pairs = [(o, _t(c).reshape(o.shape)) for o, c in zip(outputs, cotangents) if c is not None]
    total = sum((o * c).sum() for o, c in pairs)
    wanted = [x for x in inputs if x is not None]
    got = iter(torch.autograd.grad(total, wanted, allow_unused=True))
    out = []
    for x in inputs:
        if x is None:
            out.append(None)
        else:
            g = next(got)
            out.append(torch.zeros_like(x) if g is None else g)
    return out
