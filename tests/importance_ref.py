"""float64 numpy restatement of the per-Gaussian blend-contribution scores (include/r3dgs_importance.h) for
tests/test_importance_cpu.py and tests/test_importance_gpu.py, over the state of an `oracle.forward(...)["state"]` (or a
hand-built one with the same keys: xy, conic_op, point_list, ranges, n_contrib, W, H), one tile at a time with its pixels side
by side, as tests/aux_ref.py walks.

Every DECISION -- the skip of an entry, the stop -- is taken in fp32 exactly as aux_ref._walk takes it (its `take` and `stop`
expressions); every VALUE is float64: alpha = min(0.99, o exp(power)), w = alpha * T_before, T <- T (1 - alpha).  With the pixel
weight map m (None: ones), per Gaussian g:
    sum[g]   = sum of m[p] * w over the pixels p with m[p] != 0 that blend g
    max[g]   = the largest w over those pixels, 0 if none
    count[g] = the number of those pixels
No background term."""
import numpy as np

TILE = 16
F = np.float32


def scores_ref(st, weight=None, ambig=None):
    """-> dict(sum float64 [P], max float64 [P], count int64 [P], alpha_total: the float64 sum over ALL pixels of 1 - final T
    (unweighted), pairs: the number of blended (pixel, entry) pairs over ALL pixels (unweighted), ambig: bool [H*W], the
    oracle's ambiguity mask handed through (`ambig`: what oracle.forward(want_ambig=True)["ambig"] gave, or None: nothing is
    flagged) so that callers can zero the weight there)."""
    W, H = int(st["W"]), int(st["H"])
    xy32, co32 = (np.asarray(st[k], dtype=F) for k in ("xy", "conic_op"))
    xy, co = xy32.astype(np.float64), co32.astype(np.float64)
    P = len(xy32)
    plist = np.asarray(st["point_list"]).reshape(-1)
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    n_contrib = np.asarray(st["n_contrib"]).reshape(-1)
    m_all = np.ones(H * W, np.float64) if weight is None else np.asarray(weight, np.float64).reshape(-1)
    assert m_all.shape == (H * W,)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    s, mx, cnt = np.zeros(P, np.float64), np.zeros(P, np.float64), np.zeros(P, np.int64)
    alpha_total, pairs = 0.0, 0
    for tile in range(gx * gy):
        ys, xs = np.meshgrid(np.arange(TILE) + (tile // gx) * TILE, np.arange(TILE) + (tile % gx) * TILE, indexing="ij")
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        pix = ys * W + xs
        pxf, pyf = xs.astype(F), ys.astype(F)
        px, py = xs.astype(np.float64), ys.astype(np.float64)
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        n = n_contrib[pix].astype(np.int64)
        m = m_all[pix]
        counted = m != 0.0
        T32, done = np.ones(pix.shape, F), np.zeros(pix.shape, bool)
        T = np.ones(pix.shape, np.float64)
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
            # float64: the values
            ddx, ddy = xy[g, 0] - px, xy[g, 1] - py
            pw = -0.5 * (co[g, 0] * ddx * ddx + co[g, 2] * ddy * ddy) - co[g, 1] * ddx * ddy
            alpha = np.minimum(0.99, co[g, 3] * np.exp(np.minimum(pw, 0.0)))
            w = np.where(take, alpha * T, 0.0)
            T = np.where(take, T * (1.0 - alpha), T)
            pairs += int(take.sum())
            hit = take & counted
            if hit.any():
                s[g] += float((m[hit] * w[hit]).sum())
                mx[g] = max(mx[g], float(w[hit].max()))
                cnt[g] += int(hit.sum())
        alpha_total += float((1.0 - T).sum())
    flagged = np.zeros(H * W, bool) if ambig is None else (np.asarray(ambig).reshape(-1) != 0)
    return dict(sum=s, max=mx, count=cnt, alpha_total=alpha_total, pairs=pairs, ambig=flagged)
