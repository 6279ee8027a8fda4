"""numpy restatement of the auxiliary maps (include/r3dgs_aux.h) for tests/test_aux_maps_cpu.py and
tests/test_aux_maps_gpu.py, over the state of an `oracle.forward(...)["state"]` (or a hand-built one with the same keys):
xy [P,2], conic_op [P,4] (conic A, B, C and the activated opacity), depths [P], point_list, ranges [tiles,2], n_contrib [H*W],
W, H.  fp32 throughout, in the oracle's expressions (oracle/raster_oracle.c orc_blend_fwd), one tile at a time with its 256
pixels side by side.

Per pixel, over the first n_contrib entries of its tile's list: skip on power > 0 or alpha < 1/255, alpha = min(0.99,
opacity * exp(power)), T <- T (1 - alpha);
    depth        = sum of z alpha T_before over the blended entries (list order; not normalised, no background term)
    alpha        = 1 - T
    median_depth = z of the first blended entry after which T < 0.5, 0 if none
and 0 everywhere for a pixel with n_contrib == 0.  `median_ambig` flags the pixels where some T after a blended entry lies
within `ambig_rel` (relative; 1e-4 is the oracle's own default) of 0.5: there the last bit of T picks the Gaussian."""
import numpy as np

TILE = 16
F = np.float32


def blend_counts(st):
    """n_contrib [H*W] and final_T [H*W] by the reference's stop rule (forward.cu:547-552: a pixel is done at the first
    entry that would leave T < 0.0001), for a hand-built state; an oracle state carries its own."""
    return _walk(st, None, 1e-4)[3:5]


def aux_ref(st, ambig_rel=1e-4):
    """-> dict(depth, alpha, median_depth: float32 [H,W]; median_ambig: bool [H,W]; final_T float32 [H,W]; last uint32 [H,W])"""
    depth, median, ambig, last, T = _walk(st, np.asarray(st["n_contrib"]).reshape(-1), ambig_rel)
    H, W = st["H"], st["W"]
    return dict(depth=depth.reshape(H, W), alpha=(F(1.0) - T).reshape(H, W), median_depth=median.reshape(H, W),
                median_ambig=ambig.reshape(H, W), final_T=T.reshape(H, W), last=last.reshape(H, W))


def _walk(st, n_contrib, ambig_rel):
    W, H = int(st["W"]), int(st["H"])
    xy, co, z = (np.asarray(st[k], dtype=F) for k in ("xy", "conic_op", "depths"))
    plist = np.asarray(st["point_list"]).reshape(-1)
    ranges = np.asarray(st["ranges"]).reshape(-1, 2)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    depth, median, T_out = np.zeros(H * W, F), np.zeros(H * W, F), np.ones(H * W, F)
    ambig, last_out = np.zeros(H * W, bool), np.zeros(H * W, np.uint32)
    for tile in range(gx * gy):
        ys, xs = np.meshgrid(np.arange(TILE) + (tile // gx) * TILE, np.arange(TILE) + (tile % gx) * TILE, indexing="ij")
        keep = (ys < H) & (xs < W)
        ys, xs = ys[keep], xs[keep]
        pix = ys * W + xs
        pxf, pyf = xs.astype(F), ys.astype(F)
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        n = np.full(pix.shape, r1 - r0, np.int64) if n_contrib is None else n_contrib[pix].astype(np.int64)
        T, D, med = np.ones(pix.shape, F), np.zeros(pix.shape, F), np.zeros(pix.shape, F)
        crossed, done, amb = np.zeros(pix.shape, bool), np.zeros(pix.shape, bool), np.zeros(pix.shape, bool)
        last = np.zeros(pix.shape, np.uint32)
        depth_of_walk = int(n.max()) if n.size else 0
        for k in range(min(depth_of_walk, r1 - r0)):
            g = int(plist[r0 + k])
            dx, dy = xy[g, 0] - pxf, xy[g, 1] - pyf
            power = F(-0.5) * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            with np.errstate(over="ignore"):
                alpha = np.minimum(F(0.99), co[g, 3] * np.exp(power))
            take = (k < n) & ~done & (power <= F(0.0)) & (alpha >= F(1.0 / 255.0))
            Tn = T * (F(1.0) - alpha)
            stop = take & (Tn < F(0.0001))
            done |= stop
            take &= ~stop
            D = np.where(take, D + z[g] * alpha * T, D)
            T = np.where(take, Tn, T)
            last = np.where(take, np.uint32(k + 1), last)
            amb |= take & (np.abs(T - F(0.5)) <= F(ambig_rel) * F(0.5))
            cross = take & ~crossed & (T < F(0.5))
            med = np.where(cross, z[g], med)
            crossed |= cross
        depth[pix], median[pix], T_out[pix], ambig[pix], last_out[pix] = D, med, T, amb, last
    return depth, median, ambig, last_out, T_out


# The two seeded scenes of the GPU tests (tests/test_aux_maps_gpu.py; their flagged shares are measured on the CPU in
# tests/test_aux_maps_cpu.py).  A: partial tiles on both axes, mixed degrees.  B: a scene of 3 x 2 tiles just large enough that its
# heaviest tile list is at least 2 * 128 entries long (about 300), the length from which the forward leaves segment checkpoints (common.h
# kBwdSegMinLog2): a walk of several 64-entry chunks per tile.
SCENE_A = dict(P=2000, W=100, H=70, f=80.0, cam_seed=3, gseed=22, degree_mode="mixed", scale_mu=0.05)
SCENE_B = dict(P=700, W=40, H=24, f=30.0, cam_seed=5, gseed=23, degree_mode="mixed", scale_mu=0.12)


SCENE_17 = dict(P=300, W=17, H=17, f=15.0, cam_seed=2, gseed=8, degree_mode="mixed", scale_mu=0.08)   # one pixel past a tile
# Small models on a 17x19 image (partial tiles on both axes).  SCENE_65: one Gaussian past a 64-lane wave; 274 pixels blended, 10.5 %
# of them with a median depth.  SCENE_1: one Gaussian over 13 pixels, alpha up to 0.87 (one pixel below T = 0.5).  Measured with the
# CPU oracle: no threshold-ambiguous pixel in either.
SCENE_65 = dict(SCENE_17, P=65, W=19, H=17)
SCENE_1 = dict(SCENE_17, P=1, W=19, H=17, gseed=11)
SMALL = dict(P65_17x19=SCENE_65, P1_17x19=SCENE_1)
PORTRAIT = dict(camera="portrait_far", P=1500, seed=3)   # tests/camera_cases.py: fx != fy, portrait, far-rotated


def make_scene(kw):
    """-> (camera, gaussians, background) of a scene dict."""
    import synth_scene as ss
    cam = ss.make_camera(kw["W"], kw["H"], kw["f"], kw["cam_seed"])
    g = ss.make_gaussians(kw["P"], cam, seed=kw["gseed"], degree_mode=kw["degree_mode"], scale_mu=kw["scale_mu"])
    return cam, g, np.array([0.1, 0.3, 0.2], np.float32)


def hand_state(entries, W=TILE, H=TILE):
    """A one-tile state from [(x, y, A, B, C, opacity, z)] in list order (n_contrib by the reference's stop rule)."""
    e = np.asarray(entries, dtype=F).reshape(-1, 7)
    st = dict(W=W, H=H, xy=e[:, 0:2].copy(), conic_op=e[:, 2:6].copy(), depths=e[:, 6].copy(),
              point_list=np.arange(len(e), dtype=np.uint32), ranges=np.array([[0, len(e)]], np.uint32))
    st["n_contrib"], st["final_T"] = blend_counts(st)
    return st
