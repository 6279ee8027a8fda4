"""CPU pins of tests/normals_chain_ref.py, the float64 statement of the normal-consistency training step that
tests/test_normals_chain_gpu.py holds the HIP step to.  The composition is checked four ways -- against the piecewise float64
references every unit already has (at 1e-10 of max|ref|), against central finite differences of its own loss, raw against
activated leaves chained by hand, and the mip maps with a zero filter against the plain chain -- and every named scene is held
to its caps and margins with the oracle alone.  No GPU needed."""
import numpy as np
import pytest
import torch

from tests import aux_grad_ref as agr
from tests import feature_ref as fr
from tests import normals_chain_ref as ncr
from tests import normals_ref as nr

F32 = np.float32
EXACT = 1e-10   # float64 autograd of the same formulas, summed in another order
_CACHE = {}


def state_of(name, mip=False):
    """(scene, state, ambig, weight, mip dict) of a named scene over the oracle's own rects; once per scene, never modified."""
    key = (name, mip)
    if key not in _CACHE:
        sc = ncr.scene(name)
        m = opacity = scales = rows = None
        if mip:
            m, opacity, scales, rows = ncr.mip_of(sc)
        st, amb = ncr.oracle_state(sc, opacity=opacity, scales=scales)
        _CACHE[key] = (sc, st, amb, ncr.safe_weight(amb, sc.H, sc.W), m, rows)
    return _CACHE[key][:5]


def features_of(sc, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (sc.P, 2)).astype(F32), rng.uniform(-1, 1, (2, sc.H, sc.W)) / (sc.H * sc.W)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mip", [("tiny", False), ("portrait", False), ("landscape", False), ("landscape", True)])
def test_caps_and_margins_of_the_named_scenes(name, mip):
    sc, st, amb, weight, m = state_of(name, mip)
    flagged, off, w = ncr.check_scene(sc, st, amb, mip=m)
    print(f"normals chain: scene {name}{' + mip' if mip else ''}: {int((st['radii'] > 0).sum())} of {sc.P} visible, flagged {flagged:.4f} "
          f"(cap {ncr.MAX_AMBIGUOUS}), weight 0 on {off:.4f} (cap {ncr.MAX_UNWEIGHTED})")
    assert np.array_equal(w, weight) and set(np.unique(w)) <= {0.0, 1.0}
    if name == "tiny":
        assert sc.W <= 24 and sc.H <= 16 and sc.P <= 40
    if name == "portrait":
        assert (sc.W, sc.H, sc.P) == (117, 203, 600) and abs(sc.cam.tanfovx / sc.W * sc.H / sc.cam.tanfovy - 1) >= 0.2
    if mip:
        seen = st["radii"] > 0
        rows = _CACHE[(name, mip)][5]
        assert not rows[seen].any(), "a visible Gaussian sits on a decision of the mip maps"
        # render() hands the normals the FILTERED fp32 log-scales: the smallest must stay the smallest there by far more than
        # fp32 rounding (2.4e-7 at |log s| < 4), or the two sides would pick different axes
        f = m["filter_3d"].astype(F32)
        ls_eff = (F32(0.5) * np.log(np.exp(F32(2.0) * sc.g["scaling_raw"]) + f * f)).astype(F32)
        assert np.array_equal(np.argmin(ls_eff, 1)[seen], np.argmin(sc.g["scaling_raw"], 1)[seen])
        two = np.sort(ls_eff[seen].astype(np.float64), axis=1)
        assert (two[:, 1] - two[:, 0]).min() >= 1e-5 and (f[seen] > 0).all()


def test_safe_weight_is_the_three_by_three_dilation():
    amb = np.zeros((6, 9), np.uint8)
    amb[0, 0] = amb[3, 5] = 1
    w = ncr.safe_weight(amb, 6, 9)
    want = np.ones((6, 9), F32)
    want[0:2, 0:2] = 0
    want[2:5, 4:7] = 0
    assert w.dtype == F32 and np.array_equal(w, want)
    assert ncr.safe_weight(np.zeros(54), 6, 9).all()


# ---- the composition against the piecewise references ----------------------------------------------------------------------------

@pytest.mark.parametrize("scale_by_alpha", [True, False])
@pytest.mark.parametrize("name", ["tiny", "portrait"])
def test_the_chain_is_the_sum_of_the_piecewise_references(name, scale_by_alpha):
    """dL/d normal_map, dL/d depth and dL/d alpha from normals_ref at the chain's own maps, fed to aux_grad_ref.reference_grads
    and feature_ref.reference_grads; the feature reference's dL/d features is the normals' upstream, pulled through
    normals_ref.gaussian_normals to the rotation.  The three shares add up to chain_grads."""
    sc, st, _, weight, _ = state_of(name)
    g, cam, H, W = sc.g, sc.cam, sc.H, sc.W
    arrays = ncr.arrays_of(sc, False)
    whole = ncr.chain_grads(st, arrays, cam, H, W, raw=False, scale_by_alpha=scale_by_alpha, pixel_weight=weight)
    with torch.no_grad():
        maps = ncr.chain_maps(st, ncr.as_leaves(arrays), cam, H, W, raw=False)
    N, d, a = (maps[k].clone().requires_grad_(True) for k in ("normal", "depth", "alpha"))
    L, _ = nr.normal_consistency(N, d, a, cam.tanfovx, cam.tanfovy, scale_by_alpha, nr._t(weight))
    gN, gd, ga = (t.numpy() for t in torch.autograd.grad(L, (N, d, a)))
    assert abs(float(L.detach()) - whole["loss"]) <= 1e-14
    view = (cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy)
    aux = agr.reference_grads(st, g["means3D"], g["opacity"], g["scales"], g["rotations"], *view, g_depth=gd, g_alpha=ga)
    q = nr._t(g["rotations"]).requires_grad_(True)
    n = nr.gaussian_normals(nr._t(g["means3D"]), nr._t(g["scales"]), q, nr._t(cam.world_view_transform), nr._t(cam.camera_center))
    feat = fr.reference_grads(st, g["means3D"], g["opacity"], g["scales"], g["rotations"], *view, n.detach().numpy(), gN.reshape(3, -1))
    own, = torch.autograd.grad(n, q, nr._t(feat["features"]))
    parts = dict(means3D=(aux, feat), opacity=(aux, feat), scales=(aux, feat), rotations=(aux, feat, dict(rotations=own.numpy())))
    for k, shares in parts.items():
        for share in shares:
            assert np.abs(share[k]).max() > 0, f"{k}: a route carries nothing"
        total = sum(np.asarray(share[k], np.float64).reshape(whole[k].shape) for share in shares)
        top, err = np.abs(total).max(), np.abs(whole[k] - total).max()
        print(f"normals chain: {name} scale_by_alpha={scale_by_alpha}: {k}: chain against the piecewise sum {err / top:.2e} of max|ref| (bar {EXACT})")
        assert err <= EXACT * top, (k, err, top)


# ---- finite differences of the reference's own loss --------------------------------------------------------------------------------

FD_STEP = 1e-5
FD_PICKS = 20


@pytest.mark.parametrize("scale_by_alpha", [False, True])
@pytest.mark.parametrize("mip", [False, True])
def test_central_finite_differences_of_the_loss(mip, scale_by_alpha):
    """chain_grads against (L(x + h) - L(x - h)) / 2h of chain_loss in float64 on `tiny`, raw leaves, two feature channels in
    front of the normals, 20 random elements of every leaf among the visible Gaussians.

    The step and the bar come from the loss.  One evaluation of L (about 1.0, a sum of 384 pixel terms) is good to a few eps:
    the quotient carries a rounding error of about 8 eps |L| / h.  Its truncation error h^2 |L'''| / 6 is measured, not
    guessed: a second quotient at 2h differs from the first by three times it (Richardson).  At h = 1e-4 the truncation
    dominates (up to 2e-7 of max|grad|), at 1e-6 the rounding (2e-8); h = 1e-5 sits where they cross, and there
        |quotient - autograd| <= 8 eps |L| / h + 2 |quotient(2h) - quotient(h)| / 3
    is asserted per element; the bar itself must stay below 1e-6 of the tensor's largest gradient so that it cannot go
    vacuous.  Observed: at most 3.5e-9 of max|grad| (opacity), bars 4.1e-8 and below.

    Two conventions make a term of the step NOT the derivative of its value, and the scene keeps clear of both (asserted):
    the straight-through min(0.99, alpha) and the clamped-frustum Jacobian.  scale_by_alpha multiplies by alpha AS A CONSTANT;
    since w (1 - s x) = (w s)(1 - x) + w (1 - s), its gradient is that of the unscaled loss under the weight w * alpha, and
    that is the function differentiated numerically for it."""
    sc, st, _, weight, m = state_of("tiny", mip)
    cam, H, W = sc.cam, sc.H, sc.W
    seen = np.flatnonzero(st["radii"] > 0)
    assert (1 / (1 + np.exp(-sc.g["opacity"].astype(np.float64)))).max() < 0.99, "the 0.99 cap must stay out of reach"
    from tests import camera_cases as cc
    assert cc.clamped_fraction(sc.g, cam, st["radii"] > 0) == 0.0, "no visible centre past the EWA clamp"
    arrays = ncr.arrays_of(sc, True)
    arrays["features"], up = features_of(sc)
    got = ncr.chain_grads(st, arrays, cam, H, W, raw=True, scale_by_alpha=scale_by_alpha, pixel_weight=weight, feature_upstream=up, mip=m)
    fd_weight = weight
    if scale_by_alpha:
        with torch.no_grad():
            fd_weight = weight * ncr.chain_maps(st, ncr.as_leaves(arrays), cam, H, W, raw=True, mip=m)["alpha"].numpy()
    base = {k: np.array(v, np.float64).reshape(got[k].shape) for k, v in arrays.items()}

    def loss(k, i, delta):
        a = dict(base)
        a[k] = base[k].copy()
        a[k][i] += delta
        with torch.no_grad():
            leaves = {n: torch.from_numpy(v) for n, v in a.items()}
            return float(ncr.chain_loss(st, leaves, cam, H, W, raw=True, scale_by_alpha=False, pixel_weight=fd_weight,
                                        features=leaves["features"], feature_upstream=up, mip=m))
    L0 = abs(loss("opacity", (0, 0), 0.0))
    rounding = 8 * np.finfo(np.float64).eps * L0 / FD_STEP
    rng = np.random.default_rng(11)
    h = FD_STEP
    for k in base:
        top = np.abs(got[k]).max()
        assert top > 0, k
        worst = worst_bar = 0.0
        for _ in range(FD_PICKS):
            i = (int(rng.choice(seen)), int(rng.integers(base[k].shape[1])))
            q1 = (loss(k, i, h) - loss(k, i, -h)) / (2 * h)
            q2 = (loss(k, i, 2 * h) - loss(k, i, -2 * h)) / (4 * h)
            bar = rounding + 2 * abs(q2 - q1) / 3
            err = abs(q1 - got[k][i])
            assert err <= bar, f"{k}{i}: autograd {got[k][i]:.12e}, quotient {q1:.12e}: {err:.3e} > {bar:.3e}"
            worst, worst_bar = max(worst, err / top), max(worst_bar, bar / top)
        print(f"normals chain: finite differences, mip={mip} scale_by_alpha={scale_by_alpha}: {k}: worst {worst:.2e} of max|grad|, "
              f"largest bar {worst_bar:.2e}")
        assert worst_bar <= 1e-6, (k, worst_bar)


# ---- raw against activated leaves; the mip maps with nothing to do ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "portrait"])
def test_raw_leaves_equal_activated_leaves_chained_by_hand(name):
    """d/d log s = s d/ds;  d/d q = (I - u u^T) / |q| d/du with u = q / |q|: written out, not left to autograd."""
    sc, st, _, weight, _ = state_of(name)
    kw = dict(scale_by_alpha=True, pixel_weight=weight)
    raw = ncr.chain_grads(st, ncr.arrays_of(sc, True), sc.cam, sc.H, sc.W, raw=True, **kw)
    q = sc.g["rotation_raw"].astype(np.float64)
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    s = np.exp(sc.g["scaling_raw"].astype(np.float64))
    # the activated leaves are the float64 activations of the fp32 raw parameters: the two chains then see the same numbers
    act = ncr.as_leaves(ncr.arrays_of(sc, False))
    act["scales"], act["rotations"] = torch.from_numpy(s).requires_grad_(True), torch.from_numpy(q / norm).requires_grad_(True)
    L = ncr.chain_loss(st, act, sc.cam, sc.H, sc.W, raw=False, **kw)
    act = ncr.grads_of(L, act)
    u = q / norm
    by_hand = dict(means3D=act["means3D"], opacity=act["opacity"], scales=act["scales"] * s,
                   rotations=(act["rotations"] - u * (u * act["rotations"]).sum(1, keepdims=True)) / norm)
    assert abs(raw["loss"] - act["loss"]) <= 1e-14
    for k, want in by_hand.items():
        top, err = np.abs(want).max(), np.abs(raw[k] - want).max()
        print(f"normals chain: {name}: raw against activated by hand: {k} {err / top:.2e} of max|ref| (bar {EXACT})")
        assert top > 0 and err <= EXACT * top, (k, err, top)


def test_the_mip_maps_with_a_zero_filter_are_the_plain_chain():
    sc, st, _, weight, _ = state_of("tiny")
    kw = dict(raw=True, scale_by_alpha=True, pixel_weight=weight)
    plain = ncr.chain_grads(st, ncr.arrays_of(sc, True), sc.cam, sc.H, sc.W, **kw)
    zero = ncr.chain_grads(st, ncr.arrays_of(sc, True), sc.cam, sc.H, sc.W, mip=dict(filter_3d=np.zeros((sc.P, 1), F32), antialiasing=False), **kw)
    for k in plain:
        assert np.array_equal(plain[k], zero[k]), k
    # and they are not a no-op otherwise: the filters change the loss and every gradient
    m = ncr.mip_of(sc)[0]
    for mip in (m, dict(m, antialiasing=False)):
        on = ncr.chain_grads(st, ncr.arrays_of(sc, True), sc.cam, sc.H, sc.W, mip=mip, **kw)
        assert all(not np.allclose(on[k], plain[k], rtol=1e-6, atol=0) for k in plain), "a filter left a gradient as it was"
