"""Cameras that synth_scene.make_camera never builds, shared by the CPU pins of the oracle and tests/test_camera_cases_gpu.py:
non-square pixels (fx != fy: the product keeps focal_x / focal_y, the Jacobian's two rows and the two clamp limits apart),
portrait images, and view rotations far from the identity (a 360 degree capture looks at the scene from behind, from above
and rolled), with a camera centre far from the origin (what the SH direction is formed from).

A plain helper module, not a conftest.  Every entry of CAMERAS has two sizes: `cpu` -- a few tiles, for the dense fp64
autograd statement -- and `gpu` -- several whole tiles plus partial tiles in both directions, no larger than 203 x 117.
The cloud of a case is drawn in the camera frame (synth_scene.make_gaussians for the identity camera with the same
intrinsics) and carried into the world through the inverse view matrix, so every camera has the cloud in front of it."""
import math

import numpy as np

import synth_scene as ss

PI = math.pi
# name -> sizes (W, H, fx, fy), euler angles of synth_scene.rot_xyz, translation T, spread (> 1.3 pushes centres past the
# EWA clamp's 1.3 tan(fov / 2)) and, where it is not make_gaussians' 2 .. 12, the depth range of the cloud
CAMERAS = {
    # fx != fy alone: the rotation is as small as make_camera's
    "aniso": dict(cpu=(56, 40, 45.0, 61.0), gpu=(203, 117, 163.0, 221.0), euler=(0.05, -0.08, 0.03), T=(0.1, -0.2, 0.15),
                  spread=1.0),
    # portrait, non-square pixels, every off-diagonal term of the view matrix large
    "portrait_far": dict(cpu=(40, 56, 61.0, 38.0), gpu=(117, 203, 178.0, 124.0), euler=(2.5, -1.9, 1.2), T=(0.7, -1.1, 0.4),
                         spread=1.0),
    # a 90 degree roll (view x is world y), wide field of view, centres past the clamp: limx / limy far from W : H.  A
    # clamped centre lies at least 0.3 W / 2 (0.3 H / 2) pixels outside the image, and a Gaussian that touches no tile is
    # culled: only a splat of that reach is both clamped and visible, so the cloud is near (a splat of scale 0.05 at depth
    # 0.5 .. 3 reaches 3 sigma = 4 .. 20 pixels at the gpu size)
    "roll90_wide_clamp": dict(cpu=(56, 40, 20.0, 26.0), gpu=(203, 117, 72.0, 94.0), euler=(0.0, 0.0, PI / 2),
                              T=(0.0, 0.0, 0.0), spread=1.35, depth=(0.5, 3.0)),
    # seen from behind (a rotation by pi), long focal length, camera centre 6 units from the origin
    "behind_tele": dict(cpu=(56, 40, 160.0, 120.0), gpu=(197, 115, 560.0, 420.0), euler=(0.0, PI, 0.0), T=(3.0, -2.0, 5.0),
                        spread=1.0),
}
# every entry has |fx / fy - 1| >= 0.2 at both sizes (tests/test_oracle_vs_autograd.py checks the table)


def camera(name, size):
    """-> ss.Camera of entry `name` at size 'cpu' or 'gpu'."""
    c = CAMERAS[name]
    W, H, fx, fy = c[size]
    return ss.Camera(W, H, fx, fy, ss.rot_xyz(*c["euler"]), c["T"])


def identity_camera(name, size):
    """R = I, T = 0 with the entry's intrinsics: the frame synth_scene.make_gaussians draws a cloud in."""
    W, H, fx, fy = CAMERAS[name][size]
    return ss.Camera(W, H, fx, fy)


def place_in_view(g, cam):
    """A cloud drawn for the identity camera with `cam`'s intrinsics -> the same cloud in world coordinates, where `cam`
    sees it as the identity camera did: centres through the inverse of cam.world_view_transform (row vectors, float64).
    The Gaussians' rotations stay as drawn (they are random; the view rotation then turns the splats on the screen)."""
    inv = np.linalg.inv(cam.world_view_transform.astype(np.float64))
    m = np.concatenate([g["means3D"].astype(np.float64), np.ones((len(g["means3D"]), 1))], axis=1) @ inv
    out = dict(g)
    out["means3D"] = np.ascontiguousarray(m[:, :3] / m[:, 3:4], dtype=np.float32)
    return out


def cloud(name, size, P, seed, degree_mode="mixed", scale_mu=0.05, **kw):
    """-> (camera, Gaussians in world coordinates) of entry `name`: make_gaussians in the camera frame, the entry's spread
    on the camera-frame x and y, then place_in_view (2 % of the centres lie behind the camera, as in every make_gaussians
    cloud)."""
    cam = camera(name, size)
    zmin, zmax = CAMERAS[name].get("depth", (2.0, 12.0))
    g = ss.make_gaussians(P, identity_camera(name, size), seed=seed, degree_mode=degree_mode, scale_mu=scale_mu, zmin=zmin,
                          zmax=zmax, **kw)
    g["means3D"][:, :2] *= CAMERAS[name]["spread"]
    return cam, place_in_view(g, cam)


def view_space(g, cam):
    """Centres in `cam`'s view frame (float64): what the EWA clamp compares with 1.3 tan(fov / 2)."""
    m = np.concatenate([g["means3D"].astype(np.float64), np.ones((len(g["means3D"]), 1))], axis=1)
    return (m @ cam.world_view_transform.astype(np.float64))[:, :3]


def clamped_fraction(g, cam, visible):
    """Fraction of the `visible` Gaussians whose centre the EWA clamp moves: |t.x / t.z| > 1.3 tanfovx or |t.y / t.z| >
    1.3 tanfovy."""
    t = view_space(g, cam)[visible]
    hit = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tanfovx) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tanfovy)
    return float(hit.mean()) if len(t) else 0.0
