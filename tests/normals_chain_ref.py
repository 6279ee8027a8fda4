"""The normal-consistency training step as ONE float64 autograd graph, for tests/test_normals_chain_cpu.py and
tests/test_normals_chain_gpu.py:

    out = render(view, pc, pipe, bg, aux=("depth", "alpha"), aux_grad=True, normals=True, features_geom_grad=True)
    L, _ = r3dgs_normals.normal_consistency(out["normal"], out["depth"], rs, alpha=out["alpha"])

A plain helper module, not a conftest.  Nothing is restated here: the chain is the existing float64 pieces, composed --
the activations (exp, F.normalize) when `raw`, tests/mip_ref.py's two maps when `mip` is given, aux_grad_ref.geometry,
aux_grad_ref.walk (depth, alpha), feature_ref.walk over normals_ref.gaussian_normals (positions and scales detached there, as
render() does; behind the user's features when there are some) and normals_ref.normal_consistency.  Every blend DECISION is
the state's (fp32, frozen), so the loss is a smooth function of the leaves and autograd differentiates all of it at once:
the rotation's three routes, the position's, scale's and opacity's two, depth and alpha each feeding the loss twice.

The named scenes are built FOR the step: scales and rotations are drawn so that normals_ref's margins hold at that file's
defaults (SCALE_GAP, FACING_FLOOR) on every visible Gaussian, and `safe_weight` gives the pixel weight both sides use."""
import functools
import types

import numpy as np
import torch

from tests import aux_grad_ref as agr
from tests import feature_ref as fr
from tests import mip_ref
from tests import normals_ref as nr

F32 = np.float32
DT = torch.float64
BG = np.array([0.1, 0.3, 0.2], F32)
MAX_AMBIGUOUS = 0.01   # flagged pixels (tests/test_normals_gpu.py::scene)
MAX_UNWEIGHTED = 0.10  # pixels of weight 0: the flagged ones times the 3 x 3 dilation
LEAVES = ("means3D", "opacity", "scales", "rotations")
ROTATION_GAIN = 1.3    # tests/test_aux_grad_gpu.Model stores rotations * 1.3 as the raw quaternion

_t = agr._t


# ---- the chain ------------------------------------------------------------------------------------------------------------------

def chain_maps(st, leaves, cam, H, W, *, raw, features=None, mip=None):
    """-> dict(depth [H,W], alpha [H,W], normal [3,H,W], features [C,H,W] or None) as float64 torch functions of the leaves:
    a dict of float64 tensors means3D [P,3], opacity [P,1] (the logit), scales [P,3] (log-scales when `raw`), rotations [P,4]
    (unnormalised when `raw`).  `features`: a float64 [P,C] tensor blended in front of the normals.  `mip`:
    dict(filter_3d=[P,1] array, antialiasing=bool) -- render(filter_3d=f, antialiasing=...): the 3D filter on the raw
    parameters, the per-view compensation on its result; the normals keep the unfiltered scales (s -> sqrt(s^2 + f^2) is
    monotone: the smallest stays the smallest)."""
    m, o, s, q = (leaves[k] for k in LEAVES)
    V, Pm, campos = _t(cam.world_view_transform), _t(cam.full_proj_transform), _t(cam.camera_center)
    tx, ty = float(cam.tanfovx), float(cam.tanfovy)
    n = nr.gaussian_normals(m.detach(), s.detach(), q, V, campos, raw=raw)
    if mip is not None:
        ls, o = mip_ref.filtered(s if raw else torch.log(s), o, _t(mip["filter_3d"]))
        s = ls if raw else torch.exp(ls)
        if mip.get("antialiasing", False):
            o, _, _ = mip_ref.opacity(m, o, s, q, None, V, tx, ty, W, H, 1.0, raw=raw)
    scales, rotations = (torch.exp(s), torch.nn.functional.normalize(q)) if raw else (s, q)
    xy, co, z = agr.geometry(m, o, scales, rotations, V, Pm, W, H, tx, ty)
    aux = agr.walk(st, xy, co, z)
    C = 0 if features is None else int(features.shape[1])
    blended = fr.walk(st, xy, co, n if features is None else torch.cat((features, n), dim=1))
    return dict(depth=aux["depth"].reshape(H, W), alpha=aux["alpha"].reshape(H, W), normal=blended[C:].reshape(3, H, W),
                features=blended[:C].reshape(C, H, W) if C else None)


def loss_of_maps(maps, cam, *, scale_by_alpha, pixel_weight, feature_upstream=None):
    """normals_ref.normal_consistency over the maps of chain_maps, plus (feature_map * feature_upstream).sum()."""
    L, _ = nr.normal_consistency(maps["normal"], maps["depth"], maps["alpha"], float(cam.tanfovx), float(cam.tanfovy), scale_by_alpha,
                                 None if pixel_weight is None else _t(pixel_weight))
    if maps["features"] is not None:
        L = L + (maps["features"] * _t(feature_upstream).reshape(maps["features"].shape)).sum()
    return L


def chain_loss(st, leaves, cam, H, W, *, raw, scale_by_alpha, pixel_weight, features=None, feature_upstream=None, mip=None):
    """The float64 loss of the step as a torch function of the float64 leaves (chain_maps), `features` among them when given."""
    maps = chain_maps(st, leaves, cam, H, W, raw=raw, features=features, mip=mip)
    return loss_of_maps(maps, cam, scale_by_alpha=scale_by_alpha, pixel_weight=pixel_weight, feature_upstream=feature_upstream)


def as_leaves(arrays):
    """float64 leaves that require grad from a dict of fp32 arrays (LEAVES, and `features` when present)."""
    out = {k: _t(arrays[k]).requires_grad_(True) for k in LEAVES}
    out["opacity"] = _t(np.asarray(arrays["opacity"]).reshape(-1, 1)).requires_grad_(True)
    if arrays.get("features") is not None:
        out["features"] = _t(arrays["features"]).requires_grad_(True)
    return out


def grads_of(loss, leaves):
    """-> dict(loss=float, one float64 numpy gradient per leaf; zeros for a leaf the loss does not reach)."""
    names = [k for k in leaves if leaves[k] is not None]
    got = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True, retain_graph=True)
    out = {k: (torch.zeros_like(leaves[k]) if g is None else g).numpy() for k, g in zip(names, got)}
    out["loss"] = float(loss.detach())
    return out


def chain_grads(st, arrays, cam, H, W, *, raw, scale_by_alpha, pixel_weight, feature_upstream=None, mip=None):
    """chain_loss and its gradient with respect to every leaf, from a dict of fp32 arrays (as_leaves) -> grads_of's dict."""
    leaves = as_leaves(arrays)
    L = chain_loss(st, leaves, cam, H, W, raw=raw, scale_by_alpha=scale_by_alpha, pixel_weight=pixel_weight,
                   features=leaves.get("features"), feature_upstream=feature_upstream, mip=mip)
    return grads_of(L, leaves)


def safe_weight(ambig, H, W):
    """The [H,W] fp32 pixel weight of the loss on BOTH sides: 0 where the pixel or one of its eight neighbours is flagged
    threshold-ambiguous (the depth normal of a pixel reads x +- 1, y +- 1), 1 elsewhere."""
    bad = np.asarray(ambig).reshape(H, W) != 0
    pad = np.pad(bad, 1)
    near = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            near |= pad[dy:dy + H, dx:dx + W]
    return (~near).astype(F32)


# ---- the named scenes -------------------------------------------------------------------------------------------------------------

LANDSCAPE = dict(P=3000, W=160, H=112, f=130.0, cam_seed=4, gseed=31, degree_mode="mixed", scale_mu=0.05)   # test_normals_gpu.py::scene
PORTRAIT = dict(camera="portrait_far", P=600, seed=3)
TINY = dict(P=40, W=24, H=16, f=20.0, cam_seed=7, gseed=41, degree_mode="mixed", scale_mu=0.3)
REDRAW_SEED = 97
REDRAW_GAP = 8 * nr.SCALE_GAP   # a row whose two smallest scales are closer than this (relative) is drawn again


def _with_margins(cam, g, opacity_max=None):
    """The cloud with the scales of the few rows that miss the gap drawn again (same distribution: the row's own scales times
    fresh log-normal factors), the raw forms tests/test_aux_grad_gpu.Model stores, and normals_ref.with_facing_margin."""
    g = dict(g)
    rng = np.random.default_rng(REDRAW_SEED)
    scales = g["scales"].astype(np.float64)
    for _ in range(64):
        s = np.sort(scales, axis=1)
        bad = (s[:, 1] - s[:, 0]) < REDRAW_GAP * s[:, 1]
        if not bad.any():
            break
        scales[bad] *= np.exp(rng.normal(0.0, 0.3, (int(bad.sum()), 3)))
    g["scales"] = scales.astype(F32)
    if opacity_max is not None:
        g["opacity"] = np.minimum(g["opacity"], F32(opacity_max))
    g["scaling_raw"] = np.log(g["scales"]).astype(F32)
    g["rotation_raw"] = (g["rotations"] * ROTATION_GAIN).astype(F32)
    g.update(viewmatrix=cam.world_view_transform.astype(F32), campos=cam.camera_center.astype(F32))
    return nr.with_facing_margin(g)


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> namespace(name, cam, g, H, W, P) of "landscape", "portrait" or "tiny"; built once, shared, never modified."""
    if name == "portrait":
        from tests import camera_cases as cc
        cam, g = cc.cloud(PORTRAIT["camera"], "gpu", PORTRAIT["P"], PORTRAIT["seed"])
        H, W = cam.image_height, cam.image_width
    else:
        from tests import aux_ref as ar
        kw = dict(landscape=LANDSCAPE, tiny=TINY)[name]
        cam, g, _ = ar.make_scene(kw)
        H, W = kw["H"], kw["W"]
    # tiny is differentiated numerically: sigmoid(4) = 0.982 keeps every alpha below the 0.99 cap, whose straight-through
    # gradient is by design not the derivative of the clamped value
    g = _with_margins(cam, g, opacity_max=4.0 if name == "tiny" else None)
    return types.SimpleNamespace(name=name, cam=cam, g=g, H=H, W=W, P=len(g["means3D"]))


def arrays_of(sc, raw, g=None):
    """The fp32 arrays of the scene's leaves (as_leaves' input)."""
    g = sc.g if g is None else g
    return dict(means3D=g["means3D"], opacity=g["opacity"], scales=g["scaling_raw" if raw else "scales"],
                rotations=g["rotation_raw" if raw else "rotations"])


def oracle_state(sc, rects_of=None, opacity=None, scales=None):
    """The oracle's forward of the scene -> (state, ambig [H,W]).  rects_of(radii) -> the device's [P,4] rects, or None (the
    reference's own squares); opacity / scales: the effective fp32 parameters of an anti-aliased render."""
    from oracle import oracle as orc
    g, cam = sc.g, sc.cam
    out = orc.forward(BG, g["means3D"], None, g["opacity"] if opacity is None else opacity, g["scales"] if scales is None else scales,
                      g["rotations"], 1.0, None, cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, sc.H,
                      sc.W, g["sh"], g["degrees"], cam.camera_center, want_ambig=True)
    rects = None if rects_of is None else rects_of(out["radii"])
    if rects is not None:
        out = orc.with_rects(out, rects, want_ambig=True)
    return out["state"], out["ambig"]


def mip_of(sc, antialiasing=True):
    """The float64 statement of the two filters over the scene's one camera -> (mip dict for chain_maps, effective fp32 raw
    opacity [P,1], effective fp32 scales [P,3], ambiguous rows [P] bool): what the CPU file builds its state from."""
    cam, g = sc.cam, sc.g
    row = np.concatenate([cam.world_view_transform.astype(F32).reshape(16),
                          np.array([sc.W / (2.0 * cam.tanfovx), sc.H / (2.0 * cam.tanfovy), sc.W, sc.H], F32)])
    f, amb_f = mip_ref.filter3d(g["means3D"], row[None, :])
    f = f.numpy().astype(F32)
    with torch.no_grad():
        ls, o = mip_ref.filtered(_t(g["scaling_raw"]), _t(g["opacity"]), _t(f))
        amb = amb_f
        if antialiasing:
            o, _, amb_o = mip_ref.opacity(_t(g["means3D"]), o, ls, _t(g["rotation_raw"]), None, _t(cam.world_view_transform),
                                          float(cam.tanfovx), float(cam.tanfovy), sc.W, sc.H, 1.0, raw=True)
            amb = amb | amb_o
    return dict(filter_3d=f, antialiasing=antialiasing), o.numpy().astype(F32), np.exp(ls.numpy()).astype(F32), amb.numpy()


def check_scene(sc, st, ambig, maps=None, arrays=None, mip=None):
    """Every property a scene must have before a comparison over it means anything -> (flagged share, share of weight 0,
    weight [H,W]): the caps, normals_ref's Gaussian margins at the file's defaults on the visible Gaussians (both forms), and
    its image margins on the reference depth and alpha."""
    H, W, g = sc.H, sc.W, sc.g
    flagged = float((np.asarray(ambig) != 0).mean())
    weight = safe_weight(ambig, H, W)
    off = float((weight == 0).mean())
    assert flagged <= MAX_AMBIGUOUS, f"{sc.name}: {flagged:.4f} of the pixels are threshold-ambiguous"
    assert off <= MAX_UNWEIGHTED, f"{sc.name}: {off:.4f} of the pixels get weight 0"
    seen = np.asarray(st["radii"]) > 0
    assert seen.sum() >= min(20, sc.P // 2), f"{sc.name}: only {int(seen.sum())} Gaussians are visible"
    vis = {k: (v if k in ("viewmatrix", "campos") else v[seen]) for k, v in g.items() if k in
           ("means3D", "scales", "scaling_raw", "rotations", "rotation_raw", "viewmatrix", "campos")}
    for raw in (False, True):
        nr.check_margins_gaussians(vis, raw)
    if maps is None:
        with torch.no_grad():
            maps = chain_maps(st, as_leaves(arrays_of(sc, True) if arrays is None else arrays), sc.cam, H, W, raw=True, mip=mip)
    depth, alpha = maps["depth"].detach().numpy(), maps["alpha"].detach().numpy()
    c2 = nr.check_margins_image(depth, alpha, sc.cam.tanfovx, sc.cam.tanfovy)
    assert (c2 > 0).mean() >= 0.5, f"{sc.name}: the depth normal is zero on half of the image"
    return flagged, off, weight
