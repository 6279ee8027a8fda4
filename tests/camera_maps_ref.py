"""The float64 reference of the maps' share of a camera gradient (include/r3dgs_camera.h r3dgs_camera_backward_maps and the
_screen map backwards), for tests/test_camera_maps_cpu.py and tests/test_camera_maps_gpu.py.

torch.autograd.grad of sum(g * map) with respect to float64 viewmatrix and projmatrix (the transposed, row-vector matrices
the library takes, as independent inputs), through tests/aux_grad_ref.geometry -- a torch function of both matrices -- and the
existing walks: aux_grad_ref.walk (depth / alpha / median depth), distortion_ref.walk, feature_ref.walk.  Decisions are frozen
in fp32 over the state's own arrays, as those modules freeze them.  A plain helper module, not a conftest."""
import numpy as np
import torch

from tests import aux_grad_ref as agr
from tests import camera_grad_ref as cgr
from tests import distortion_ref as dr
from tests import feature_ref as fr

DT = torch.float64


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def loss_of(st, xy, co, z, up):
    """sum(g * map) over the maps named in `up`: depth / alpha / median_depth -> g [H*W]; distortion -> (g [H*W], near, far);
    features -> (F [P,C], g [C,H*W]).  float64 torch."""
    loss = torch.zeros((), dtype=DT)
    if any(k in up for k in ("depth", "alpha", "median_depth")):
        maps = agr.walk(st, xy, co, z)
        for k in ("depth", "alpha", "median_depth"):
            if up.get(k) is not None:
                loss = loss + (T(np.asarray(up[k]).reshape(-1)) * maps[k]).sum()
    if up.get("distortion") is not None:
        g, near, far = up["distortion"]
        loss = loss + (T(np.asarray(g).reshape(-1)) * dr.walk(st, xy, co, z, near, far)["distortion"]).sum()
    if up.get("features") is not None:
        F, g = up["features"]
        loss = loss + (T(np.asarray(g).reshape(F.shape[1], -1)) * fr.walk(st, xy, co, T(F))).sum()
    return loss


def camera_grads(st, g, cam, up, V=None, Fm=None, state_values=False):
    """-> dict of numpy float64: viewmatrix [4,4], projmatrix [4,4] (the partial derivatives of the loss, the two matrices
    independent), and the per-Gaussian screen-space gradients of the same loss in the LIBRARY's units -- means2D [P,2] (pixel
    mean times 0.5 W / 0.5 H), conic [P,3] (A, B, C with B halved: the colour backward's convention, backward.cu's -0.5 on all
    three where d power / dB = -dx dy), z [P] -- and loss.  V, Fm: other matrices than the camera's (finite differences).
    state_values: the walk reads the VALUES of the state's own fp32 xy, conic_op and depths (what the library's passes read) and
    the geometry supplies the derivatives alone: what the fp32 forward state is worth against end-to-end float64."""
    W, H = int(st["W"]), int(st["H"])
    V = T(cam.world_view_transform if V is None else V).requires_grad_(True)
    Fm = T(cam.full_proj_transform if Fm is None else Fm).requires_grad_(True)
    xy, co, z = agr.geometry(T(g["means3D"]), T(np.asarray(g["opacity"]).reshape(-1, 1)), T(g["scales"]), T(g["rotations"]), V, Fm,
                             W, H, cam.tanfovx, cam.tanfovy)
    if state_values:
        xy, co, z = (T(st[k]).reshape(t.shape) + (t - t.detach()) for k, t in (("xy", xy), ("conic_op", co), ("depths", z)))
    sxy, sco, sz = (torch.zeros_like(t, requires_grad=True) for t in (xy, co, z))
    loss = loss_of(st, xy + sxy, co + sco, z + sz, up) + 0.0 * (sxy.sum() + sco.sum() + sz.sum() + V.sum() + Fm.sum())
    gV, gF, gxy, gco, gz = torch.autograd.grad(loss, (V, Fm, sxy, sco, sz))
    conic = gco[:, :3].numpy() * np.array([1.0, 0.5, 1.0])
    return dict(viewmatrix=gV.numpy(), projmatrix=gF.numpy(), means2D=gxy.numpy() * np.array([0.5 * W, 0.5 * H]), conic=conic,
                z=gz.numpy(), loss=float(loss.detach()))


def chained(g, cam, per_gaussian, radii, cov3D):
    """The two partial derivatives from GIVEN per-Gaussian screen-space gradients (library units: means2D, conic, z of
    `camera_grads`) and a given cov3D [P,6], through the per-Gaussian stage alone: what r3dgs_camera_backward_maps computes, in
    float64 and with the conventions r3dgs_camera_backward documents (fp32 focal lengths and clamp limits, 1 / (det^2 + 1e-7)) --
    tests/camera_grad_ref.camera_grads, the colour route's pinned reference of the same chain -- plus the maps' own term:
    z = (mt V)_2, so dL/dV[k, 2] += dL_dz * mt[k]."""
    W, H = cam.image_width, cam.image_height
    P = len(g["means3D"])
    conic = np.asarray(per_gaussian["conic"], np.float64)
    gcon = np.stack([conic[:, 0], conic[:, 1], np.zeros(P), conic[:, 2]], 1)
    out = cgr.camera_grads(g["means3D"], cov3D, None, None, radii, cam.world_view_transform, cam.full_proj_transform, np.zeros(3),
                           W, H, cam.tanfovx, cam.tanfovy, per_gaussian["means2D"], gcon, None)
    vis = np.asarray(radii).reshape(-1) > 0
    mt = np.concatenate([np.asarray(g["means3D"], np.float64), np.ones((P, 1))], 1)
    gv = out["viewmatrix"].copy()
    gv[:, 2] += (mt[vis] * np.asarray(per_gaussian["z"], np.float64).reshape(-1)[vis, None]).sum(0)
    return dict(viewmatrix=gv, projmatrix=out["projmatrix"])
