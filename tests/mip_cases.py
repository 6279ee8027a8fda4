"""Seeded scenes for the anti-aliasing tests (tests/test_mip_cpu.py, tests/test_mip_gpu.py): fp32 numpy arrays, the same on the
CPU and on the GPU.  Per scene a tenth of the Gaussians lies behind the near plane, a tenth are needles (scale ratio 1e3), a
tenth are sub-pixel (most of them under the 0.000025 floor of the compensation) and the raw opacities spread over +-15."""
import math

import numpy as np

F32 = np.float32
W, H = 64, 48
TAN_FOVX, TAN_FOVY = 0.55, 0.35   # focal_x = 58.2, focal_y = 68.6: not square pixels


def view_matrix(angle=0.3, axis=(0.2, 1.0, 0.1), shift=(0.1, -0.2, 4.0)):
    """world_view_transform as the renderer passes it: [4,4], a point is a row vector on its left (translation in row 3)."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    V = np.eye(4)
    V[:3, :3] = R
    V[3, :3] = shift
    return V.astype(F32)


def scene(P, seed=0, view=None):
    rng = np.random.default_rng(seed)
    V = view_matrix() if view is None else view
    Vd = V.astype(np.float64)
    z = rng.uniform(1.0, 8.0, P)
    kind = np.arange(P) % 10   # 0: behind the near plane, 1: needle, 2: sub-pixel
    rng.shuffle(kind)
    z[kind == 0] = rng.uniform(-2.0, 0.19, int((kind == 0).sum()))
    # up to 1.6 x the field of view: the 1.3 tan(fov) clamp acts on some rows
    tv = np.stack([rng.uniform(-1.6, 1.6, P) * TAN_FOVX * np.abs(z), rng.uniform(-1.6, 1.6, P) * TAN_FOVY * np.abs(z), z], 1)
    means = ((tv - Vd[3, :3]) @ Vd[:3, :3].T).astype(F32)
    scales = np.exp(rng.uniform(-4.0, -1.0, (P, 3)))
    n = kind == 1
    long_axis = np.exp(rng.uniform(-1.0, 0.0, int(n.sum())))
    scales[n] = long_axis[:, None] * 1e-3
    scales[n, rng.integers(0, 3, int(n.sum()))] = long_axis
    s = kind == 2
    scales[s] = np.exp(rng.uniform(math.log(1e-5), math.log(5e-3), (int(s.sum()), 3)))
    q = rng.normal(0, 1, (P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    opac = rng.uniform(-15.0, 15.0, (P, 1))
    if P >= 4:
        opac[:2, 0] = (15.0, -15.0)
    out = {"means3D": means, "opacities": opac.astype(F32), "scales": scales.astype(F32), "rotations": q.astype(F32),
           "scaling_raw": np.log(scales).astype(F32), "rotation_raw": (q * 10.0 ** rng.uniform(-1, 1, (P, 1))).astype(F32),
           "viewmatrix": V, "kind": kind}
    # the precomputed covariance of the activated pair (6 floats: 00,01,02,11,12,22), as the model's get_covariance forms it
    sc, qq = out["scales"].astype(np.float64), out["rotations"].astype(np.float64)
    r, x, y, zq = qq.T
    R = np.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y), 2 * (x * y + r * zq),
                  1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x), 2 * (x * zq - r * y), 2 * (y * zq + r * x),
                  1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    M = R * sc[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    out["cov3D"] = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(F32)
    return out


def cameras(V, seed=0, portrait_pair=True):
    """[V,20] camera table: rows of world_view_transform (16), focal_x, focal_y, W, H.  The first two are a 64x48 landscape /
    48x64 portrait pair with fx != fy; the rest look at the scene from around it."""
    rng = np.random.default_rng(1000 + seed)
    rows = []
    for v in range(V):
        M = view_matrix(angle=0.3 + 0.25 * v * (1 if v % 2 else -1), axis=(0.2 + 0.1 * (v % 3), 1.0, 0.1 * (v % 5)),
                        shift=(0.1 - 0.05 * (v % 4), -0.2 + 0.03 * (v % 7), 4.0 + 0.2 * (v % 6)))
        w, h = (W, H) if v % 2 == 0 else (H, W)
        fx, fy = w / (2 * TAN_FOVX) * (1 + 0.1 * rng.random()), h / (2 * TAN_FOVY) * (1 + 0.1 * rng.random())
        rows.append(np.concatenate([M.reshape(16), [fx, fy, w, h]]))
    return np.asarray(rows, F32).reshape(V, 20)


def filter_values(P, seed=0):
    """A [P,1] filter with exact zeros in it (a fifth of the rows) and sizes around the scales'."""
    rng = np.random.default_rng(2000 + seed)
    f = np.exp(rng.uniform(-7.0, -1.0, (P, 1)))
    f[rng.random((P, 1)) < 0.2] = 0.0
    return f.astype(F32)
