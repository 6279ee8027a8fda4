"""float64 torch restatement of tests/aux_ref.py's walk, differentiable in xy, conic_op and depths, for
tests/test_aux_grad_cpu.py and tests/test_aux_grad_gpu.py: the reference of r3dgs_aux_maps_backward (include/r3dgs_aux.h).

Over the same state dictionary as aux_ref (xy, conic_op, depths, point_list, ranges, n_contrib, W, H).  Every DECISION -- the
skip of an entry, the stop, the median's selection -- is taken in fp32 exactly as aux_ref._walk takes it and frozen; every
VALUE is float64 torch, with alpha = min(0.99, o G) straight-through as the reference's backward has it (oracle/torch_ref.py):
    depth = sum z alpha T_before,  alpha = 1 - T_final,  median_depth = z of the selected entry (0: none).
`reference_grads` = torch.autograd.grad of sum(g_D depth + g_A alpha + g_M median) through `geometry`, the per-Gaussian
geometry from means3D, scales, rotations and the raw opacity written out in float64 from oracle/torch_ref.py's expressions."""
import numpy as np
import torch

TILE = 16
F = np.float32
DT = torch.float64


def geometry(means3D, opacity_raw, scales, rotations, viewmatrix, projmatrix, W, H, tan_fovx, tan_fovy, scale_modifier=1.0,
             cov3D_precomp=None):
    """-> (xy [P,2], conic_op [P,4], depths [P]) as float64 torch functions of the float64 inputs (oracle/torch_ref.py
    render(): projection, EWA covariance with the clamped-frustum convention of the reference's backward, +0.3 dilation,
    conic, sigmoid opacity; the view depth is the third component of the view-space mean)."""
    P = means3D.shape[0]
    V, Fm = viewmatrix.to(DT), projmatrix.to(DT)
    ones = torch.ones(P, 1, dtype=DT)
    t = torch.cat([means3D, ones], 1) @ V
    h = torch.cat([means3D, ones], 1) @ Fm
    pw = 1.0 / (h[:, 3] + 1e-7)
    mx = ((h[:, 0] * pw + 1.0) * W - 1.0) * 0.5
    my = ((h[:, 1] * pw + 1.0) * H - 1.0) * 0.5
    if cov3D_precomp is None:
        r, x, y, z = rotations[:, 0], rotations[:, 1], rotations[:, 2], rotations[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        L = R * (scales * scale_modifier)[:, None, :]
        Sigma = L @ L.transpose(1, 2)
    else:
        c = cov3D_precomp
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    fx, fy = W / (2.0 * tan_fovx), H / (2.0 * tan_fovy)
    tz = t[:, 2]
    limx, limy = 1.3 * tan_fovx, 1.3 * tan_fovy
    txc = torch.clamp(t[:, 0] / tz, -limx, limx) * tz
    tyc = torch.clamp(t[:, 1] / tz, -limy, limy) * tz
    tx_var = torch.where((t[:, 0] / tz).abs() > limx, txc.detach(), t[:, 0])
    ty_var = torch.where((t[:, 1] / tz).abs() > limy, tyc.detach(), t[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx_var) / (tz * tz), zero, fy / tz, -(fy * ty_var) / (tz * tz)], 1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].t()
    cov = A @ Sigma @ A.transpose(1, 2)
    a, b, c_ = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c_ - b * b
    det = torch.where(det != 0, det, torch.ones_like(det))
    o = torch.sigmoid(opacity_raw.reshape(-1))
    return torch.stack([mx, my], 1), torch.stack([c_ / det, -b / det, a / det, o], 1), tz


def walk(st, xy, conic_op, depths):
    """The maps as float64 torch functions of xy [P,2], conic_op [P,4], depths [P] (float64 tensors; rows of Gaussians the
    lists do not name are never read), with aux_ref._walk's fp32 decisions over the state's own fp32 arrays.
    -> dict(depth, alpha, median_depth: float64 [H*W])"""
    W, H = int(st["W"]), int(st["H"])
    xy32, co32, z32 = (np.asarray(st[k], dtype=F) for k in ("xy", "conic_op", "depths"))
    plist = np.asarray(st["point_list"]).reshape(-1)
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    n_contrib = np.asarray(st["n_contrib"]).reshape(-1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    depth_parts, alpha_parts, median_parts, pix_parts = [], [], [], []
    for tile in range(gx * gy):
        ys, xs = np.meshgrid(np.arange(TILE) + (tile // gx) * TILE, np.arange(TILE) + (tile % gx) * TILE, indexing="ij")
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        pix = ys * W + xs
        pxf, pyf = xs.astype(F), ys.astype(F)
        px, py = torch.from_numpy(xs.astype(np.float64)), torch.from_numpy(ys.astype(np.float64))
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        n = n_contrib[pix].astype(np.int64)
        T32 = np.ones(pix.shape, F)
        crossed, done = np.zeros(pix.shape, bool), np.zeros(pix.shape, bool)
        T = torch.ones(len(pix), dtype=DT)
        D, med = torch.zeros(len(pix), dtype=DT), torch.zeros(len(pix), dtype=DT)
        for k in range(min(int(n.max()) if n.size else 0, r1 - r0)):
            g = int(plist[r0 + k])
            # fp32, as aux_ref._walk: the decisions
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
            cross = take & ~crossed & (T32 < F(0.5))
            crossed |= cross
            if not take.any():
                continue
            # float64, differentiable: the values
            tk = torch.from_numpy(take)
            ddx, ddy = xy[g, 0] - px, xy[g, 1] - py
            pw = -0.5 * (conic_op[g, 0] * ddx * ddx + conic_op[g, 2] * ddy * ddy) - conic_op[g, 1] * ddx * ddy
            araw = conic_op[g, 3] * torch.exp(torch.clamp(pw, max=0.0))
            alpha = araw + (torch.clamp(araw, max=0.99) - araw).detach()   # straight-through min(0.99, .)
            alpha = torch.where(tk, alpha, torch.zeros_like(alpha))
            D = D + depths[g] * alpha * T
            T = T * (1.0 - alpha)
            if cross.any():
                med = torch.where(torch.from_numpy(cross), depths[g].expand_as(med), med)
        depth_parts.append(D)
        alpha_parts.append(1.0 - T)
        median_parts.append(med)
        pix_parts.append(torch.from_numpy(pix.astype(np.int64)))
    index = torch.cat(pix_parts)
    out = {}
    for name, parts in (("depth", depth_parts), ("alpha", alpha_parts), ("median_depth", median_parts)):
        out[name] = torch.zeros(H * W, dtype=DT).index_put((index,), torch.cat(parts))
    return out


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def state_grads(st, g_depth=None, g_alpha=None, g_median=None):
    """Gradients of sum(g_D depth + g_A alpha + g_M median) with respect to the state's own xy, conic_op (conic A, B, C and
    the activated opacity) and depths -> dict(xy [P,2], conic_op [P,4], depths [P], maps=the float64 maps), numpy."""
    xy, co, z = (_t(st[k]).requires_grad_(True) for k in ("xy", "conic_op", "depths"))
    maps = walk(st, xy, co, z)
    loss = _loss(maps, st, g_depth, g_alpha, g_median) + 0.0 * z.sum()   # (attached even when no pixel selects anything)
    gxy, gco, gz = torch.autograd.grad(loss, (xy, co, z), allow_unused=True)
    zeros = lambda g, like: (torch.zeros_like(like) if g is None else g).numpy()   # noqa: E731
    return dict(xy=zeros(gxy, xy), conic_op=zeros(gco, co), depths=zeros(gz, z), maps={k: v.detach().numpy() for k, v in maps.items()})


def _loss(maps, st, g_depth, g_alpha, g_median):
    loss = torch.zeros((), dtype=DT)
    for name, g in (("depth", g_depth), ("alpha", g_alpha), ("median_depth", g_median)):
        if g is not None:
            loss = loss + (_t(np.asarray(g).reshape(-1)) * maps[name]).sum()
    return loss


def reference_grads(st, means3D, opacity_raw, scales, rotations, viewmatrix, projmatrix, tan_fovx, tan_fovy, g_depth=None,
                    g_alpha=None, g_median=None, scale_modifier=1.0, cov3D_precomp=None):
    """The reference of r3dgs_aux_maps_backward -> dict of numpy float64 arrays: means3D [P,3], opacity [P,1] (raw), scales
    [P,3], rotations [P,4] (or cov3D [P,6]), means2D [P,2] (the gradient of the pixel mean times 0.5 W / 0.5 H, the units the
    library's dL_dmeans2D has) and z [P] (the gradient of the view depth alone: the z sum)."""
    W, H = int(st["W"]), int(st["H"])
    m3, op = _t(means3D).requires_grad_(True), _t(np.asarray(opacity_raw).reshape(-1, 1)).requires_grad_(True)
    sc = rot = cov = None
    if cov3D_precomp is None:
        sc, rot = _t(scales).requires_grad_(True), _t(rotations).requires_grad_(True)
    else:
        cov = _t(cov3D_precomp).requires_grad_(True)
    xy, co, z = geometry(m3, op, sc, rot, _t(viewmatrix), _t(projmatrix), W, H, tan_fovx, tan_fovy, scale_modifier, cov)
    shift = torch.zeros_like(xy, requires_grad=True)   # in pixels; its gradient is dL / d(pixel mean)
    zshift = torch.zeros_like(z, requires_grad=True)
    maps = walk(st, xy + shift, co, z + zshift)
    loss = _loss(maps, st, g_depth, g_alpha, g_median) + 0.0 * zshift.sum()
    leaves = [m3, op, shift, zshift] + ([sc, rot] if cov is None else [cov])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [(torch.zeros_like(leaf) if g is None else g).numpy() for g, leaf in zip(grads, leaves)]
    out = dict(means3D=grads[0], opacity=grads[1], means2D=grads[2] * np.array([0.5 * W, 0.5 * H]), z=grads[3])
    if cov is None:
        out.update(scales=grads[4], rotations=grads[5])
    else:
        out.update(cov3D=grads[4])
    out["maps"] = {k: v.detach().numpy() for k, v in maps.items()}
    return out
