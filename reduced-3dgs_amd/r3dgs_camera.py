"""r3dgs_camera -- a camera whose pose can be refined by gradient descent through the rasterizer.

    from r3dgs_camera import RefinedCamera
    cam = RefinedCamera(camera)                       # any camera render() accepts (scene/cameras.py Camera)
    opt = torch.optim.Adam([cam.xi], lr=1e-3)
    loss = l1(render(cam, gaussians, pipe, bg)["render"], photo); loss.backward(); opt.step()

`xi` is a [6] parameter: a rotation vector (radians) and a translation (scene units) in the camera's own frame; zero is the
camera as given.  The three tensors the rasterizer reads are built from it on the device, from elementwise torch operations and
small matrix products only -- no host wait: exp is written in closed form (se3_exp below), not through torch.linalg.matrix_exp,
which copies a norm to the host to choose its approximation -- in the reference's transposed (row-vector) convention:
    world_view_transform = W0 @ exp(xi)^T        exp: the matrix exponential of the 4x4 twist [[w]x, v; 0, 0]
    full_proj_transform  = world_view_transform @ projection_matrix
    camera_center        = inverse(world_view_transform)[3, :3]
so a point's view coordinates become exp(xi) applied to what the given camera saw.  Because they require grad, render() takes the
camera-differentiable route (include/r3dgs_camera.h: partial derivatives with respect to the three tensors as independent
inputs) and autograd chains the three through the lines above into xi.grad.  Every other attribute render() reads
(image_height, image_width, FoVx, FoVy, ...) is passed through from the wrapped camera; the field of view is not refined.

Each access of one of the three properties rebuilds it from the current xi.  `snapshot()` evaluates the three once and returns
a plain camera object holding them; r3dgs_render.render takes a snapshot of a camera that offers one, so a render builds the
pose once however often it looks at the camera."""
import torch
import torch.nn as nn


def _as_matrix(m, device):
    return torch.as_tensor(m, dtype=torch.float32).detach().to(device).reshape(4, 4).clone()


def se3_exp(xi):
    """[6] (w, v) -> exp of the 4x4 twist [[w]x, v; 0, 0] in closed form: R = I + A K + B K^2 (Rodrigues), t = (I + B K + C K^2) v
    with K = [w]x, th = |w|, A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3.  Below th^2 = 1e-2 the three are
    taken from their series in th^2 (the next term is below 1e-13), so xi = 0 has a finite value and a finite gradient; the other
    branch is evaluated on a th^2 kept away from zero, so that the branch not taken never hands autograd a NaN."""
    w, v = xi[:3], xi[3:]
    t = torch.dot(w, w)
    small = t < 1e-2
    A_s = 1.0 - t / 6.0 + t * t / 120.0 - t * t * t / 5040.0
    B_s = 0.5 - t / 24.0 + t * t / 720.0 - t * t * t / 40320.0
    C_s = 1.0 / 6.0 - t / 120.0 + t * t / 5040.0 - t * t * t / 362880.0
    tc = torch.clamp(t, min=1e-2)
    th = torch.sqrt(tc)
    A = torch.where(small, A_s, torch.sin(th) / th)
    B = torch.where(small, B_s, (1.0 - torch.cos(th)) / tc)
    C = torch.where(small, C_s, (th - torch.sin(th)) / (tc * th))
    z = xi.new_zeros(())
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    R = eye + A * K + B * K2
    tr = (eye + B * K + C * K2) @ v
    top = torch.cat([R, tr[:, None]], dim=1)
    return torch.cat([top, torch.cat([z.expand(3), z.new_ones(1)])[None, :]], dim=0)


class _Snapshot:
    """The three pose tensors of a RefinedCamera evaluated once, every other attribute passed through."""

    def __init__(self, camera, world_view_transform, full_proj_transform, camera_center):
        self._camera = camera
        self.world_view_transform, self.full_proj_transform, self.camera_center = world_view_transform, full_proj_transform, camera_center

    def __getattr__(self, name):
        return getattr(self.__dict__["_camera"], name)


class RefinedCamera(nn.Module):
    def __init__(self, camera, device=None):
        super().__init__()
        self.__dict__["_camera"] = None
        w0 = camera.world_view_transform
        if device is None:
            device = w0.device if isinstance(w0, torch.Tensor) else torch.device("cuda")
        self.register_buffer("W0", _as_matrix(w0, device))
        self.register_buffer("projection_matrix", _as_matrix(camera.projection_matrix, device))
        self.xi = nn.Parameter(torch.zeros(6, dtype=torch.float32, device=device))
        self.__dict__["_camera"] = camera   # not a submodule, not a buffer: what __getattr__ below falls back to

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)   # parameters, buffers, submodules
        except AttributeError:
            return getattr(self.__dict__["_camera"], name)

    @property
    def world_view_transform(self):
        return self.W0 @ se3_exp(self.xi).t()

    @property
    def full_proj_transform(self):
        return self.world_view_transform @ self.projection_matrix

    @property
    def camera_center(self):
        return self.center_of(self.world_view_transform)

    def snapshot(self):
        """The pose built once from the current xi -> a camera object holding the three tensors (attached to xi)."""
        wv = self.world_view_transform
        return _Snapshot(self, wv, wv @ self.projection_matrix, self.center_of(wv))

    @staticmethod
    def center_of(world_view_transform):
        """inverse(world_view_transform)[3, :3] for a matrix [[A, 0], [b, 1]]: -b A^-1, the 3x3 inverse by cofactors."""
        a, b = world_view_transform[:3, :3], world_view_transform[3, :3]
        r0, r1, r2 = a[0], a[1], a[2]
        c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
        inv = torch.stack([c0, c1, c2], dim=1) / torch.dot(r0, c0)
        return -(b @ inv)

    def pose_error(self, world_view_transform):
        """(angle in radians, distance of the camera centres) between this camera and a world_view_transform given in the
        same convention."""
        mine, other = self.world_view_transform.detach(), _as_matrix(world_view_transform, self.W0.device)
        rel = mine[:3, :3].t() @ other[:3, :3]
        angle = torch.acos(((rel.diagonal().sum() - 1.0) * 0.5).clamp(-1.0, 1.0))
        return float(angle), float((self.center_of(mine) - self.center_of(other)).norm())
