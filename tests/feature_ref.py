"""float64 torch restatement of the feature maps (include/r3dgs_features.h) for tests/test_feature_maps_cpu.py and
tests/test_feature_maps_gpu.py: tests/aux_grad_ref.py's walk with C feature channels where it has the view depth.

Over the same state dictionary as aux_ref / aux_grad_ref (xy, conic_op, point_list, ranges, n_contrib, W, H).  Every DECISION
-- the skip of an entry, the stop -- is taken in fp32 exactly as aux_grad_ref.walk takes it and frozen; every VALUE is float64
torch, with alpha = min(0.99, o G) straight-through:
    feat[c, pixel] = sum_k F[id_k, c] alpha_k T_before_k          (no background term, no normalisation)
`reference_grads` = torch.autograd.grad of sum(g * feat) through aux_grad_ref.geometry, as aux_grad_ref.reference_grads."""
import numpy as np
import torch

from tests import aux_grad_ref as agr

TILE = agr.TILE
F = np.float32
DT = torch.float64


def walk(st, xy, conic_op, feats):
    """The map as a float64 torch function of xy [P,2], conic_op [P,4] and feats [P,C] -> float64 [C, H*W], with
    aux_grad_ref.walk's fp32 decisions over the state's own fp32 arrays."""
    W, H = int(st["W"]), int(st["H"])
    C = int(feats.shape[1])
    xy32, co32 = (np.asarray(st[k], dtype=F) for k in ("xy", "conic_op"))
    plist = np.asarray(st["point_list"]).reshape(-1)
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    n_contrib = np.asarray(st["n_contrib"]).reshape(-1)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    parts, pix_parts = [], []
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
        done = np.zeros(pix.shape, bool)
        T = torch.ones(len(pix), dtype=DT)
        D = torch.zeros(len(pix), C, dtype=DT)
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
            if not take.any():
                continue
            # float64, differentiable: the values
            tk = torch.from_numpy(take)
            ddx, ddy = xy[g, 0] - px, xy[g, 1] - py
            pw = -0.5 * (conic_op[g, 0] * ddx * ddx + conic_op[g, 2] * ddy * ddy) - conic_op[g, 1] * ddx * ddy
            araw = conic_op[g, 3] * torch.exp(torch.clamp(pw, max=0.0))
            alpha = araw + (torch.clamp(araw, max=0.99) - araw).detach()   # straight-through min(0.99, .)
            alpha = torch.where(tk, alpha, torch.zeros_like(alpha))
            D = D + (alpha * T)[:, None] * feats[g][None, :]
            T = T * (1.0 - alpha)
        parts.append(D)
        pix_parts.append(torch.from_numpy(pix.astype(np.int64)))
    index = torch.cat(pix_parts)
    return torch.zeros(H * W, C, dtype=DT).index_put((index,), torch.cat(parts)).t().contiguous()


_t = agr._t


def feature_map(st, features):
    """-> numpy float64 [C, H*W]: the map alone, over the state's own xy and conic_op."""
    with torch.no_grad():
        return walk(st, _t(st["xy"]), _t(st["conic_op"]), _t(features)).numpy()


def state_grads(st, features, g_out):
    """Gradients of sum(g_out * feat) with respect to the state's own xy and conic_op and to the features -> dict(xy [P,2],
    conic_op [P,4], features [P,C], map=[C,H*W]), numpy."""
    xy, co, f = (_t(a).requires_grad_(True) for a in (st["xy"], st["conic_op"], features))
    m = walk(st, xy, co, f)
    loss = (_t(np.asarray(g_out).reshape(m.shape)) * m).sum() + 0.0 * f.sum()
    gs = torch.autograd.grad(loss, (xy, co, f), allow_unused=True)
    zeros = lambda g, like: (torch.zeros_like(like) if g is None else g).numpy()   # noqa: E731
    return dict(xy=zeros(gs[0], xy), conic_op=zeros(gs[1], co), features=zeros(gs[2], f), map=m.detach().numpy())


def reference_grads(st, means3D, opacity_raw, scales, rotations, viewmatrix, projmatrix, tan_fovx, tan_fovy, features, g_out,
                    scale_modifier=1.0, cov3D_precomp=None):
    """The reference of r3dgs_feature_maps_backward -> dict of numpy float64 arrays: features [P,C], means3D [P,3], opacity
    [P,1] (raw), scales [P,3], rotations [P,4] (or cov3D [P,6]), means2D [P,2] (the gradient of the pixel mean times 0.5 W /
    0.5 H, the units the library's dL_dmeans2D has) and map [C,H*W]."""
    W, H = int(st["W"]), int(st["H"])
    m3, op = _t(means3D).requires_grad_(True), _t(np.asarray(opacity_raw).reshape(-1, 1)).requires_grad_(True)
    f = _t(features).requires_grad_(True)
    sc = rot = cov = None
    if cov3D_precomp is None:
        sc, rot = _t(scales).requires_grad_(True), _t(rotations).requires_grad_(True)
    else:
        cov = _t(cov3D_precomp).requires_grad_(True)
    xy, co, _ = agr.geometry(m3, op, sc, rot, _t(viewmatrix), _t(projmatrix), W, H, tan_fovx, tan_fovy, scale_modifier, cov)
    shift = torch.zeros_like(xy, requires_grad=True)   # in pixels; its gradient is dL / d(pixel mean)
    m = walk(st, xy + shift, co, f)
    loss = (_t(np.asarray(g_out).reshape(m.shape)) * m).sum() + 0.0 * f.sum()
    leaves = [m3, op, shift, f] + ([sc, rot] if cov is None else [cov])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [(torch.zeros_like(leaf) if g is None else g).numpy() for g, leaf in zip(grads, leaves)]
    out = dict(means3D=grads[0], opacity=grads[1], means2D=grads[2] * np.array([0.5 * W, 0.5 * H]), features=grads[3])
    if cov is None:
        out.update(scales=grads[4], rotations=grads[5])
    else:
        out.update(cov3D=grads[4])
    out["map"] = m.detach().numpy()
    return out
