"""float64 torch reference of the depth-distortion map and its gradients (include/r3dgs_distortion.h) for
tests/test_distortion_cpu.py and tests/test_distortion_gpu.py, over the state dictionary of tests/aux_ref.py (xy, conic_op,
depths, point_list, ranges, n_contrib, W, H).

Every DECISION -- the skip of an entry, the stop -- is taken in fp32 exactly as aux_ref._walk / aux_grad_ref.walk take it and
frozen; every VALUE is float64 torch, alpha = min(0.99, o G) straight-through:
    w_k = alpha_k T_before_k,   m_k = z_k  (near = far = 0)   or   far / (far - near) (1 - near / z_k)  (0 < near < far)
    distortion = sum_k w_k (m_k^2 A_<k + D2_<k - 2 m_k D1_<k)          (the prefix form, on the UNSHIFTED mapped depths)
`reference_grads` = torch.autograd.grad of sum(g * distortion) through aux_grad_ref.geometry.

`shifted_fp32` is an fp32 numpy restatement of what the kernel does -- fp32 weights and shifted mapped depths, the running sums
in `acc` precision -- by which the CPU tests show the GPU value bar to be reachable."""
import numpy as np
import torch

from tests import aux_grad_ref as agr

TILE = 16
F = np.float32
DT = torch.float64


def mapped(z, near, far):
    """The mapped depth of (torch or numpy, float64) view depths."""
    if near == 0.0 and far == 0.0:
        return z
    assert 0.0 < near < far
    return far / (far - near) * (1.0 - near / z)


def _tiles(st):
    W, H = int(st["W"]), int(st["H"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    n_contrib = np.asarray(st["n_contrib"]).reshape(-1)
    for tile in range(gx * gy):
        ys, xs = np.meshgrid(np.arange(TILE) + (tile // gx) * TILE, np.arange(TILE) + (tile % gx) * TILE, indexing="ij")
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        pix = ys * W + xs
        yield pix, xs, ys, int(ranges[tile, 0]), int(ranges[tile, 1]), n_contrib[pix].astype(np.int64)


def _decisions(st):
    """Per tile: (pix, xs, ys, [(Gaussian id, take mask)] for the entries some pixel blends), aux_ref._walk's fp32 decisions."""
    xy32, co32 = (np.asarray(st[k], dtype=F) for k in ("xy", "conic_op"))
    plist = np.asarray(st["point_list"]).reshape(-1)
    for pix, xs, ys, r0, r1, n in _tiles(st):
        pxf, pyf = xs.astype(F), ys.astype(F)
        T32 = np.ones(pix.shape, F)
        done = np.zeros(pix.shape, bool)
        entries = []
        for k in range(min(int(n.max()) if n.size else 0, r1 - r0)):
            g = int(plist[r0 + k])
            dx, dy = xy32[g, 0] - pxf, xy32[g, 1] - pyf
            power = F(-0.5) * (co32[g, 0] * dx * dx + co32[g, 2] * dy * dy) - co32[g, 1] * dx * dy
            with np.errstate(over="ignore"):
                alpha32 = np.minimum(F(0.99), co32[g, 3] * np.exp(power))
            take = (k < n) & ~done & (power <= F(0.0)) & (alpha32 >= F(1.0 / 255.0))
            Tn = T32 * (F(1.0) - alpha32)
            stop = take & (Tn < F(0.0001))
            done |= stop
            take &= ~stop
            T32 = np.where(take, Tn, T32)
            if take.any():
                entries.append((g, take, alpha32))
        yield pix, xs, ys, (int(plist[r0]) if r1 > r0 else None), entries


def walk(st, xy, conic_op, depths, near=0.0, far=0.0):
    """-> dict(distortion, A, S1, S2, totals: float64 torch [H*W]) as functions of xy [P,2], conic_op [P,4], depths [P];
    `distortion` is the prefix form, `totals` = A S2 - S1^2 (the identity the backward builds on)."""
    W, H = int(st["W"]), int(st["H"])
    parts = {k: [] for k in ("distortion", "A", "S1", "S2")}
    index = []
    for pix, xs, ys, _, entries in _decisions(st):
        px, py = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
        T = torch.ones(len(pix), dtype=DT)
        A, D1, D2, dist = (torch.zeros(len(pix), dtype=DT) for _ in range(4))
        for g, take, _ in entries:
            ddx, ddy = xy[g, 0] - px, xy[g, 1] - py
            pw = -0.5 * (conic_op[g, 0] * ddx * ddx + conic_op[g, 2] * ddy * ddy) - conic_op[g, 1] * ddx * ddy
            araw = conic_op[g, 3] * torch.exp(torch.clamp(pw, max=0.0))
            alpha = araw + (torch.clamp(araw, max=0.99) - araw).detach()   # straight-through min(0.99, .)
            alpha = torch.where(torch.from_numpy(take), alpha, torch.zeros_like(alpha))
            w = alpha * T
            m = mapped(depths[g], near, far)
            dist = dist + w * (m * m * A + D2 - 2.0 * m * D1)
            A, D1, D2 = A + w, D1 + w * m, D2 + w * m * m
            T = T * (1.0 - alpha)
        for k, v in (("distortion", dist), ("A", A), ("S1", D1), ("S2", D2)):
            parts[k].append(v)
        index.append(torch.from_numpy(pix.astype(np.int64)))
    index = torch.cat(index)
    out = {k: torch.zeros(H * W, dtype=DT).index_put((index,), torch.cat(v)) for k, v in parts.items()}
    out["totals"] = out["A"] * out["S2"] - out["S1"] ** 2
    return out


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def reference_map(st, near=0.0, far=0.0):
    """-> the float64 map [H*W], numpy."""
    with torch.no_grad():
        return walk(st, _t(st["xy"]), _t(st["conic_op"]), _t(st["depths"]), near, far)["distortion"].numpy()


def state_grads(st, g, near=0.0, far=0.0):
    """Gradients of sum(g * distortion) with respect to the state's own xy, conic_op and depths -> dict, numpy."""
    xy, co, z = (_t(st[k]).requires_grad_(True) for k in ("xy", "conic_op", "depths"))
    maps = walk(st, xy, co, z, near, far)
    loss = (_t(np.asarray(g).reshape(-1)) * maps["distortion"]).sum() + 0.0 * (z.sum() + xy.sum() + co.sum())
    gxy, gco, gz = torch.autograd.grad(loss, (xy, co, z))
    return dict(xy=gxy.numpy(), conic_op=gco.numpy(), depths=gz.numpy(), map=maps["distortion"].detach().numpy())


def reference_grads(st, means3D, opacity_raw, scales, rotations, viewmatrix, projmatrix, tan_fovx, tan_fovy, g, near=0.0,
                    far=0.0, scale_modifier=1.0, cov3D_precomp=None):
    """The reference of r3dgs_distortion_map_backward -> dict of numpy float64 arrays, as aux_grad_ref.reference_grads: means3D,
    opacity (raw), scales, rotations (or cov3D), means2D (times 0.5 W / 0.5 H), z, and map = the float64 map [H*W]."""
    W, H = int(st["W"]), int(st["H"])
    m3, op = _t(means3D).requires_grad_(True), _t(np.asarray(opacity_raw).reshape(-1, 1)).requires_grad_(True)
    sc = rot = cov = None
    if cov3D_precomp is None:
        sc, rot = _t(scales).requires_grad_(True), _t(rotations).requires_grad_(True)
    else:
        cov = _t(cov3D_precomp).requires_grad_(True)
    xy, co, z = agr.geometry(m3, op, sc, rot, _t(viewmatrix), _t(projmatrix), W, H, tan_fovx, tan_fovy, scale_modifier, cov)
    shift = torch.zeros_like(xy, requires_grad=True)   # in pixels; its gradient is dL / d(pixel mean)
    zshift = torch.zeros_like(z, requires_grad=True)
    maps = walk(st, xy + shift, co, z + zshift, near, far)
    loss = (_t(np.asarray(g).reshape(-1)) * maps["distortion"]).sum() + 0.0 * zshift.sum()
    leaves = [m3, op, shift, zshift] + ([sc, rot] if cov is None else [cov])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [(torch.zeros_like(leaf) if gr is None else gr).numpy() for gr, leaf in zip(grads, leaves)]
    out = dict(means3D=grads[0], opacity=grads[1], means2D=grads[2] * np.array([0.5 * W, 0.5 * H]), z=grads[3])
    if cov is None:
        out.update(scales=grads[4], rotations=grads[5])
    else:
        out.update(cov3D=grads[4])
    out["map"] = maps["distortion"].detach().numpy()
    return out


def far_scene(P=160, W=48, H=40, f=1500.0):
    """FAR: visible depths in about 100 <= z <= 104 under a narrow field of view (f = 1500 px over 48 x 40), splats a few
    pixels wide and faint enough that a pixel blends many: raw fp32 moments (z^2 ~ 1e4, spread ~ 1) lose the answer here."""
    import synth_scene as ss
    cam = ss.make_camera(W, H, f, 1)
    g = ss.make_gaussians(P, cam, seed=9, degree_mode="mixed", scale_mu=0.05)
    rng = np.random.default_rng(10)
    Vi = np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4))
    zv = rng.uniform(100.0, 104.0, P)
    xv = (rng.uniform(-2.0, W + 1.0, P) - (W - 1) / 2) / (W / (2 * cam.tanfovx)) * zv
    yv = (rng.uniform(-2.0, H + 1.0, P) - (H - 1) / 2) / (H / (2 * cam.tanfovy)) * zv
    g["means3D"] = (np.stack([xv, yv, zv, np.ones(P)], 1) @ Vi)[:, :3].astype(np.float32)
    g["scales"] = ((2.5 / f) * zv[:, None] * rng.uniform(0.5, 1.5, (P, 3))).astype(np.float32)
    g["opacity"] = rng.uniform(-2.5, 0.0, (P, 1)).astype(np.float32)   # sigmoid: 8 % .. 50 %
    return cam, g, H, W


def stacked(P, W=32, H=32):
    """P faint Gaussians stacked over the first 16x16 tile of a 32x32 image (tests/test_aux_grad_gpu.py's construction): one
    list longer than a 64-entry chunk."""
    import synth_scene as ss
    cam = ss.make_camera(W, H, 30.0, 1)
    g = ss.make_gaussians(P, cam, seed=5, degree_mode="mixed", scale_mu=0.05)
    rng = np.random.default_rng(6)
    Vi = np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4))
    fx = W / (2 * cam.tanfovx)
    zv = rng.uniform(2.0, 6.0, P)
    xv = (rng.uniform(3.0, 12.0, P) - (W - 1) / 2) / fx * zv
    yv = (rng.uniform(3.0, 12.0, P) - (H - 1) / 2) / (H / (2 * cam.tanfovy)) * zv
    g["means3D"] = (np.stack([xv, yv, zv, np.ones(P)], 1) @ Vi)[:, :3].astype(np.float32)
    g["scales"] = (0.02 * zv[:, None] * rng.uniform(0.6, 1.4, (P, 3))).astype(np.float32)
    g["opacity"] = rng.uniform(-4.2, -3.2, (P, 1)).astype(np.float32)   # sigmoid: 1.5 % .. 4 %, a deep walk
    return cam, g, H, W


def gpu_scenes():
    """name -> (camera, gaussians, H, W, (near, far) mappings) of every scene tests/test_distortion_gpu.py holds to the
    reference; tests/test_distortion_cpu.py measures the flag share and the fp32 restatement on each."""
    from tests import aux_ref as ar
    from tests import camera_cases as cc
    cam, g, _ = ar.make_scene(ar.SCENE_A)
    yield "A", cam, g, ar.SCENE_A["H"], ar.SCENE_A["W"], ((0.0, 0.0), (0.2, 50.0))
    cam, g, _ = ar.make_scene(ar.SCENE_17)
    yield "17x17", cam, g, 17, 17, ((0.0, 0.0),)
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", 600, ar.PORTRAIT["seed"])
    yield "portrait", cam, g, cam.image_height, cam.image_width, ((0.0, 0.0),)
    for P in (512, 203):
        cam, g, H, W = stacked(P)
        yield f"stacked{P}", cam, g, H, W, ((0.0, 0.0),)
    cam, g, H, W = far_scene()
    yield "FAR", cam, g, H, W, ((0.0, 0.0),)


def shifted_fp32(st, near=0.0, far=0.0, acc=np.float64):
    """The kernel's forward restated in numpy: fp32 weights w = alpha T (aux_ref's fp32 expressions), fp32 mapped depths
    relative to the tile's first list entry, the four running sums in `acc` precision, rounded to fp32 at the end.
    -> dict(distortion, S1, S2: float32 [H*W])"""
    W, H = int(st["W"]), int(st["H"])
    z32 = np.asarray(st["depths"], dtype=F)
    k = F(0.0) if near == 0.0 else F(float(far) * float(near) / (float(far) - float(near)))
    out = {name: np.zeros(H * W, F) for name in ("distortion", "S1", "S2")}
    for pix, xs, ys, g_first, entries in _decisions(st):
        T = np.ones(pix.shape, F)
        A, D1, D2, dist = (np.zeros(pix.shape, acc) for _ in range(4))
        z_ref = z32[g_first] if g_first is not None else F(1.0)
        for g, take, alpha32 in entries:
            dz = z32[g] - z_ref
            m = acc(dz if near == 0.0 else k * dz / (z32[g] * z_ref))
            w = np.where(take, alpha32 * T, F(0.0)).astype(acc)
            wm = w * m
            wmm = wm * m
            dist = dist + (wmm * A + w * D2 - acc(2.0) * wm * D1)
            A, D1, D2 = A + w, D1 + wm, D2 + wmm
            T = np.where(take, T * (F(1.0) - alpha32), T)
        out["distortion"][pix], out["S1"][pix], out["S2"][pix] = dist.astype(F), D1.astype(F), D2.astype(F)
    return out
