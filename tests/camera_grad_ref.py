"""Float64 reference of the camera gradients (include/r3dgs_camera.h): a torch restatement of the PER-GAUSSIAN stage only --
pixel mean from projmatrix, conic from viewmatrix, colour from campos -- whose autograd maps given per-Gaussian sums
dL_dmean2D, dL_dconic ([P,4]: A, B, -, C) and dL_dcolor to dL/dviewmatrix, dL/dprojmatrix, dL/dcampos.  Written from the
maths (SURVEY.md A1-A3 and the quirks listed in oracle/torch_ref.py), not from csrc/camera_math.h.  A plain helper module.

With mt = [m, 1] (row vectors; V, F the transposed matrices as the reference passes them), per Gaussian with radii > 0:
    ndc   = (mt F).xy / ((mt F).w + 1e-7)                       dL_dmean2D is dL/dndc (the units the backward writes)
    t     = mt V;  J = [[fx / tz, 0, -fx tx / tz^2], [0, fy / tz, -fy ty / tz^2]] with tx / tz, ty / tz clamped to
            1.3 tan(fov / 2) and a clamped tx (ty) a constant times tz inside J that passes nothing on
    cov2D = (J V[:3,:3]^T) Sigma (J V[:3,:3]^T)^T + 0.3 I;  conic = cov2D^-1 = (c, -b, a) / det
            the B slot of dL_dconic holds HALF the derivative with respect to the off-diagonal (it appears twice in the
            quadratic form): loss = gA A + 2 gB B + gC C
    rgb   = max(0, sum_k Y_k(d / |d|) sh_k + 0.5), d = m - campos, k < (degree + 1)^2
pure=True: exactly that (what fp64 autograd of oracle/torch_ref.render differentiates).  pure=False: the conventions of the
product's backward on top -- fp32 focal lengths and clamp limits, dL/dcov2D scaled by det^2 / (det^2 + 1e-7) (the backward
divides by det^2 + 1e-7), and, when `clamped` is given, the forward's own colour-clamp decisions instead of this evaluation's."""
import numpy as np
import torch

from oracle import torch_ref as tr

F64 = torch.float64


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=F64)


def cov3d_of(scales, rotations, mod=1.0):
    """Sigma = R diag(mod s)^2 R^T as [P,6] (00, 01, 02, 11, 12, 22), float64, from the numbers given (no normalisation)."""
    L = tr.quat_to_R(_t(rotations)) * (_t(scales) * mod)[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).numpy()


def camera_grads(means3D, cov3D, sh, degrees, radii, viewmatrix, projmatrix, campos, W, H, tan_fovx, tan_fovy, dL_dmean2D,
                 dL_dconic, dL_dcolor, clamped=None, pure=False):
    """-> dict(viewmatrix [4,4], projmatrix [4,4], campos [3]) of float64 arrays.  sh None: precomputed colours (campos gets
    zeros).  cov3D [P,6]; dL_dmean2D [P,2 or 3]; dL_dconic [P,4] or [P,2,2]; clamped [P,3] bool / uint8 or None."""
    vis = torch.tensor(np.asarray(radii).reshape(-1) > 0)
    V, F, cp = _t(viewmatrix).reshape(4, 4).requires_grad_(), _t(projmatrix).reshape(4, 4).requires_grad_(), _t(campos).requires_grad_()
    zero = dict(viewmatrix=np.zeros((4, 4)), projmatrix=np.zeros((4, 4)), campos=np.zeros(3))
    if int(vis.sum()) == 0:
        return zero
    m = _t(means3D)[vis]
    n = m.shape[0]
    mt = torch.cat([m, torch.ones(n, 1, dtype=F64)], 1)
    g2 = _t(dL_dmean2D).reshape(len(vis), -1)[vis][:, :2]
    gcon = _t(dL_dconic).reshape(len(vis), 4)[vis]
    gA, gB, gC = gcon[:, 0], gcon[:, 1], gcon[:, 3]

    h = mt @ F
    loss = (h[:, :2] / (h[:, 3:4] + 1e-7) * g2).sum()

    t = mt @ V
    if pure:
        fx, fy, limx, limy = W / (2.0 * tan_fovx), H / (2.0 * tan_fovy), 1.3 * tan_fovx, 1.3 * tan_fovy
    else:
        f32 = np.float32
        fx, fy = float(f32(W) / (f32(2.0) * f32(tan_fovx))), float(f32(H) / (f32(2.0) * f32(tan_fovy)))
        limx, limy = float(f32(1.3) * f32(tan_fovx)), float(f32(1.3) * f32(tan_fovy))
    tz = t[:, 2]
    rx, ry = t[:, 0] / tz, t[:, 1] / tz
    tx = torch.where(rx.abs() > limx, (torch.clamp(rx, -limx, limx) * tz).detach(), t[:, 0])
    ty = torch.where(ry.abs() > limy, (torch.clamp(ry, -limy, limy) * tz).detach(), t[:, 1])
    o = torch.zeros_like(tz)
    J = torch.stack([fx / tz, o, -fx * tx / (tz * tz), o, fy / tz, -fy * ty / (tz * tz)], 1).reshape(n, 2, 3)
    A = J @ V[:3, :3].t()
    c6 = _t(cov3D)[vis]
    S = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(n, 3, 3)
    cov = A @ S @ A.transpose(1, 2)
    abc = torch.stack([cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3], 1)

    def conic_loss(x):
        a, b, c = x[:, 0], x[:, 1], x[:, 2]
        det = a * c - b * b
        ok = det != 0
        det = torch.where(ok, det, torch.ones_like(det))
        return (torch.where(ok, gA * c / det - 2.0 * gB * b / det + gC * a / det, torch.zeros_like(det))).sum()

    if pure:
        loss = loss + conic_loss(abc)
    else:
        leaf = abc.detach().requires_grad_()
        (g,) = torch.autograd.grad(conic_loss(leaf), leaf)
        det2 = (leaf[:, 0] * leaf[:, 2] - leaf[:, 1] ** 2).detach() ** 2
        loss = loss + (abc * (g * (det2 / (det2 + 1e-7))[:, None])).sum()

    if sh is not None:
        d = m - cp[None, :]
        d = d / d.norm(dim=1, keepdim=True)
        Y = tr.sh_basis(d[:, 0], d[:, 1], d[:, 2])
        K = (torch.tensor(np.asarray(degrees).reshape(-1).astype(np.int64))[vis] + 1) ** 2
        shv = _t(sh)[vis]
        M = shv.shape[1]
        kmask = (torch.arange(16)[None, :] < K[:, None]).to(F64)
        raw = ((Y * kmask)[:, :M, None] * shv).sum(1) + 0.5
        if clamped is None or pure:
            rgb = torch.clamp(raw, min=0.0)
        else:
            rgb = raw * torch.tensor(np.asarray(clamped).reshape(-1, 3) == 0)[vis].to(F64)
        loss = loss + (rgb * _t(dL_dcolor).reshape(-1, 3)[vis]).sum()
    loss.backward()
    out = dict(zero)
    for name, x in (("viewmatrix", V), ("projmatrix", F), ("campos", cp)):
        if x.grad is not None:
            out[name] = x.grad.numpy().copy()
    return out


def relerr(ref, got):
    """max |got - ref| / max |ref| (0 for two all-zero tensors)."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64).reshape(np.shape(ref))
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())
