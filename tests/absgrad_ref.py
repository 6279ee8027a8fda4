"""Float64 restatement of the absolute screen-space gradients (AbsGS), written from their definition:

    abs_x[i] = (W/2) sum over pixels | dL/dG * G * -(A dx + B dy) |,    abs_y[i] = (H/2) sum over pixels | dL/dG * G * -(C dy + B dx) |

where the term inside the bars is what the reference's backward renderCUDA adds to dL_dmean2D[i].x / .y for that pixel
(backward.cu:553-554; dL/dG = opacity * dL/dalpha, d = mean - pixel, G = exp(-0.5 (A dx^2 + C dy^2) - B dx dy)), and the sum
runs over the (pixel, entry) pairs the forward blended.  Explicit loops over tiles, list entries and (vectorised) the pixels of
a tile, in numpy; nothing of the kernels' headers is used.  The discrete decisions are taken in float32 as the forward takes
them, the values are double, as in oracle/backward_f64.c -- the signed column returned next to the abs one is held to that
file's dL_dmean2D (tests/test_absgrad_cpu.py), which pins this restatement to something that already exists."""
import numpy as np

TILE = 16
F = np.float32


def absgrad_ref(st, dL_dpix, ambig=None):
    """st: the state of oracle.forward (or hand_state below); dL_dpix [3,H,W].
    -> dict(signed [P,2] float64, abs [P,2] float64, ambig: bool [H,W] -- the oracle's threshold-ambiguous pixels, the rule of
    the parity tests, passed through; None in: none flagged)."""
    W, H = int(st["W"]), int(st["H"])
    xy32, co32 = np.asarray(st["xy"], dtype=F), np.asarray(st["conic_op"], dtype=F)
    xy, co = xy32.astype(np.float64), co32.astype(np.float64)
    colors = st.get("colors_precomp")
    colors = np.asarray(st["rgb"] if colors is None else colors, dtype=np.float64)
    bg = np.asarray(st["bg"], dtype=np.float64)
    plist = np.asarray(st["point_list"]).reshape(-1)
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    n_contrib = np.asarray(st["n_contrib"]).reshape(-1).astype(np.int64)
    g = np.asarray(dL_dpix, dtype=F).reshape(3, -1).astype(np.float64)
    P = xy.shape[0]
    signed, absol = np.zeros((P, 2)), np.zeros((P, 2))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    for tile in range(gx * gy):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        ys, xs = np.meshgrid(np.arange(TILE) + (tile // gx) * TILE, np.arange(TILE) + (tile % gx) * TILE, indexing="ij")
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        pix = ys * W + xs
        last = n_contrib[pix]
        depth = min(int(last.max()) if last.size else 0, r1 - r0)
        if depth == 0:
            continue
        pxf, pyf = xs.astype(F), ys.astype(F)
        # forward products: alpha of every (entry, pixel) (0: skipped) and the transmittance in front of it
        A_, G_, T_ = np.zeros((depth, pix.size)), np.zeros((depth, pix.size)), np.zeros((depth, pix.size))
        T = np.ones(pix.size)
        for k in range(depth):
            i = int(plist[r0 + k])
            dxf, dyf = xy32[i, 0] - pxf, xy32[i, 1] - pyf   # the decisions, in fp32 as the kernels take them
            powf = F(-0.5) * (co32[i, 0] * dxf * dxf + co32[i, 2] * dyf * dyf) - co32[i, 1] * dxf * dyf
            with np.errstate(over="ignore"):
                alphaf = np.minimum(F(0.99), co32[i, 3] * np.exp(powf))
            take = (k < last) & (powf <= F(0.0)) & (alphaf >= F(1.0 / 255.0))
            dx, dy = xy[i, 0] - pxf.astype(np.float64), xy[i, 1] - pyf.astype(np.float64)
            G = np.exp(-0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy)
            a = np.where(take, np.minimum(0.99, co[i, 3] * G), 0.0)
            A_[k], G_[k], T_[k] = a, G, T
            T = T * (1.0 - a)
        # back to front: S = colour composited behind the entry + T_end * bg
        S = T[None, :] * bg[:, None]
        for k in range(depth - 1, -1, -1):
            i = int(plist[r0 + k])
            a, Tf = A_[k], T_[k]
            on = a != 0.0
            if not on.any():
                continue
            c = colors[i]
            with np.errstate(invalid="ignore", divide="ignore"):
                dL_da = sum(g[ch, pix] * (c[ch] * Tf - S[ch] / (1.0 - a)) for ch in range(3))
            S = S + np.where(on, c[:, None] * (a * Tf)[None, :], 0.0)
            dL_dG = co[i, 3] * dL_da
            dx, dy = xy[i, 0] - pxf.astype(np.float64), xy[i, 1] - pyf.astype(np.float64)
            tx = np.where(on, dL_dG * G_[k] * -(co[i, 0] * dx + co[i, 1] * dy) * (0.5 * W), 0.0)
            ty = np.where(on, dL_dG * G_[k] * -(co[i, 2] * dy + co[i, 1] * dx) * (0.5 * H), 0.0)
            for p in range(pix.size):   # one term per (pixel, entry): signed, and under the bars
                if on[p]:
                    signed[i, 0] += tx[p]
                    signed[i, 1] += ty[p]
                    absol[i, 0] += abs(tx[p])
                    absol[i, 1] += abs(ty[p])
    flagged = np.zeros((H, W), bool) if ambig is None else np.asarray(ambig).reshape(H, W) != 0
    return dict(signed=signed, abs=absol, ambig=flagged)


def masked_upstream(dL_dpix, ambig):
    """dL_dpix with the threshold-ambiguous pixels taken out (for both sides of a comparison)."""
    out = np.array(dL_dpix, dtype=F, copy=True)
    out.reshape(3, -1)[:, np.asarray(ambig).reshape(-1) != 0] = 0.0
    return out


def hand_state(entries, colors, n_contrib, bg=(0.0, 0.0, 0.0), W=1, H=1):
    """A one-tile state from [(x, y, A, B, C, opacity)] in list order."""
    e = np.asarray(entries, dtype=F).reshape(-1, 6)
    return dict(W=W, H=H, xy=e[:, 0:2].copy(), conic_op=e[:, 2:6].copy(), rgb=np.asarray(colors, dtype=F).reshape(-1, 3),
                colors_precomp=None, bg=np.asarray(bg, dtype=F), point_list=np.arange(len(e), dtype=np.uint32),
                ranges=np.array([[0, len(e)]], np.uint32), n_contrib=np.asarray(n_contrib, np.uint32).reshape(-1))


# The seeded scenes of tests/test_absgrad_gpu.py; tests/test_absgrad_cpu.py measures their flagged shares with the oracle alone.
# TILES: 3 x 2 tiles with partial tiles on both edges.  ONE_TILE: a single tile under 200 large Gaussians -- one list of more than
# two 64-entry chunks (and, with R3DGS_BWD_SEG_LEN at its smallest, of more than one segment).
SCENE_TILES = dict(P=300, W=40, H=24, f=30.0, cam_seed=5, gseed=31, degree_mode="mixed", scale_mu=0.12)
SCENE_ONE_TILE = dict(P=200, W=16, H=16, f=14.0, cam_seed=2, gseed=32, degree_mode="mixed", scale_mu=0.25)
PORTRAIT = dict(camera="portrait_far", P=400, seed=3)   # tests/camera_cases.py: 117 x 203, fx != fy


def make_scene(kw):
    import synth_scene as ss
    cam = ss.make_camera(kw["W"], kw["H"], kw["f"], kw["cam_seed"])
    gs = ss.make_gaussians(kw["P"], cam, seed=kw["gseed"], degree_mode=kw["degree_mode"], scale_mu=kw["scale_mu"])
    return cam, gs, np.array([0.1, 0.3, 0.2], np.float32)
