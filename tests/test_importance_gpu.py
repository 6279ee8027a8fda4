"""GPU tests (-m gpu) of the per-Gaussian blend-contribution scores (include/r3dgs_importance.h, csrc/importance.hip) against
tests/importance_ref.py over the oracle re-binned into the HIP rects, against the forward's own final_T / n_contrib bit for
bit, against the feature backward and the alpha map on the device, across every forward entry point and both bindings, with
accumulation over views, at the edges, inside a captured graph and through r3dgs_importance.

Bars (the pixel weight is 0 on the oracle's threshold-ambiguous pixels on both sides; their share is at most 0.1 %):
  * count: exact;
  * max: within 1e-5 absolute -- the project's per-pixel value bar for a quantity in [0, 1];
  * sum: within 1e-5 * max(1, count[g]) per Gaussian (weights in [-1, 1]): each term is a blend weight, which the RGB bar
    already holds to 1e-5.
The overflow rule (a Gaussian that lost pairs to an overflowed reservation contributes nothing) is covered on the host by
tests/test_importance_cpu.py: the aux-gradient tests hold no state whose forward overflowed its reservation either.
"""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import camera_cases as cc
from tests import importance_ref as ir

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
FLAG_MAX_FRACTION = 1e-3
BG = np.array([0.1, 0.3, 0.2], np.float32)
NAMES = ("sum", "max", "count", "views")


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


def dev(a):
    return EMPTY if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def forward_args(g, cam, H, W, scales=None, rotations=None):
    return (dev(BG), dev(g["means3D"]), EMPTY, dev(g["opacity"]), dev(g["scales"]) if scales is None else scales,
            dev(g["rotations"]) if rotations is None else rotations, 1.0, EMPTY, dev(cam.world_view_transform),
            dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]), dev(g["degrees"]), dev(cam.camera_center),
            False, False)


def scores_of(C_, P, H, W, fout, weight=None, **kw):
    R, _, _, geom, binning, img = fout
    return C_.contribution_scores(P, R, H, W, geom, binning, img, pixel_weight=weight, **kw)


def same_scores(a, b, what):
    for k in NAMES:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)


def consistent(C_, P, H, W, fout, got):
    """T_check == final_T and n_check == n_contrib, bit for bit, on every pixel."""
    ex = C_.export_binning(P, fout[0], H, W, fout[3], fout[4], fout[5])
    assert torch.equal(got["T_check"].reshape(-1), ex["final_T"]), "the walk's own final T is not the forward's"
    assert torch.equal(got["n_check"].reshape(-1), ex["n_contrib"]), "the walk's own last contributor is not the forward's"
    return ex


def random_weight(H, W, seed):
    """[-1, 1] with zeros of both signs."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32)
    m[rng.random((H, W)) < 0.15] = 0.0
    m[rng.random((H, W)) < 0.05] = -0.0
    return m


_cases = {}


def case(C_, name):
    """The exact-size forward of a scene and the oracle's state re-binned into its rects, once per scene."""
    if name in _cases:
        return _cases[name]
    if name == "portrait_far":
        cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", ar.PORTRAIT["P"], ar.PORTRAIT["seed"])
        H, W = cam.image_height, cam.image_width
    else:
        kw = dict(ar.SMALL, A=ar.SCENE_A, B=ar.SCENE_B, s17=ar.SCENE_17)[name]
        cam, g, _ = ar.make_scene(kw)
        H, W = kw["H"], kw["W"]
    P = len(g["means3D"])
    C_.hint_next_forward(True)   # as a training step: full blob, checkpoints
    fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
    ref = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                      cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                      want_ambig=True)
    if C_.tight_rects():
        rects = C_.export_rects(P, fout[3]).cpu().numpy()
        rects[ref["radii"] <= 0] = 0
        ref = orc.with_rects(ref, rects, want_ambig=True)
    amb = (ref["ambig"] != 0).reshape(H, W)
    print(f"[importance {name}] oracle-ambiguous {100 * amb.mean():.4f} % (cap {100 * FLAG_MAX_FRACTION:.2f} %)")
    assert amb.mean() <= FLAG_MAX_FRACTION
    _cases[name] = NS(cam=cam, g=g, P=P, H=H, W=W, fout=fout, st=ref["state"], amb=amb, refs={})
    return _cases[name]


def parity(C_, name, weight_name, m, min_seen=10):
    """Every bar of the module's docstring for one scene and one weight map (None: ones) -> (case, scores)."""
    c = case(C_, name)
    m_ = np.ones((c.H, c.W), np.float32) if m is None else m.copy()
    m_[c.amb] = 0.0
    if weight_name not in c.refs:
        c.refs[weight_name] = ir.scores_ref(c.st, m_)
    want = c.refs[weight_name]
    got = scores_of(C_, c.P, c.H, c.W, c.fout, dev(m_), checks=True)
    consistent(C_, c.P, c.H, c.W, c.fout, got)
    assert [got[k].dtype for k in NAMES] == [torch.float64, torch.float32, torch.int64, torch.int32]
    s, mx, cnt, views = (got[k].cpu().numpy() for k in NAMES)
    assert (cnt == want["count"]).all(), f"{int((cnt != want['count']).sum())} counts differ"
    assert (views == (cnt > 0)).all()
    err_max = np.abs(mx - want["max"]).max()
    err_sum = (np.abs(s - want["sum"]) / np.maximum(1, cnt)).max()
    print(f"[importance {name} / {weight_name}] max err {err_max:.3e} (bar 1e-5), sum err / max(1, count) {err_sum:.3e} "
          f"(bar 1e-5), largest count {cnt.max()}, Gaussians seen {int((cnt > 0).sum())} of {c.P}")
    assert err_max <= 1e-5 and err_sum <= 1e-5
    assert (cnt > 0).sum() > min_seen and mx.max() > 0.3
    return c, got


def test_parity_scene_a(C_):
    """Scene A (P = 2000 at 100x70: partial tiles on both axes, mixed degrees)."""
    parity(C_, "A", "ones", None)


def test_parity_scene_b_long_lists(C_):
    """Scene B (P = 700 at 40x24): a tile list of at least 256 entries and a walk of more than 64, so the chunk and segment
    boundaries are crossed; the walk's final T and last contributor equal the forward's bit for bit (parity's `consistent`)."""
    c, _ = parity(C_, "B", "ones", None)
    ex = C_.export_binning(c.P, c.fout[0], c.H, c.W, c.fout[3], c.fout[4], c.fout[5])
    lens = (ex["ranges"][:, 1] - ex["ranges"][:, 0]).cpu().numpy()
    print(f"[importance B] heaviest tile list {lens.max()} entries, deepest contributor {int(ex['n_contrib'].max())}")
    assert lens.max() >= 256 and int(ex["n_contrib"].max()) > 64


@pytest.mark.parametrize("name", ["s17", "portrait_far"])
def test_parity_edge_cameras(C_, name):
    """SCENE_17 (17x17, one pixel past a tile) and PORTRAIT (fx != fy, portrait, far-rotated)."""
    parity(C_, name, "ones", None)


def test_small_models_on_a_17x19_image(C_):
    """P = 65 (one Gaussian past a wave) and P = 1 on 17x19, partial tiles on both axes.  The single Gaussian is seen (13 pixels,
    alpha * T up to 0.87): `parity` asks for it alone there, not for more than ten."""
    parity(C_, "P65_17x19", "ones", None)
    parity(C_, "P1_17x19", "ones", None, min_seen=0)


def test_weights(C_):
    """A random map with zeros of both signs and negative values against the reference; None equals a map of ones bit for
    bit; an all-zero map gives all zeros."""
    c = case(C_, "A")
    _, got = parity(C_, "A", "random", random_weight(c.H, c.W, 11))
    assert float(got["sum"].min()) < 0
    none = scores_of(C_, c.P, c.H, c.W, c.fout)
    ones = scores_of(C_, c.P, c.H, c.W, c.fout, torch.ones(c.H, c.W, device="cuda"))
    same_scores(none, ones, "None against ones")
    assert int(none["count"].sum()) > int(got["count"].sum())
    zero = scores_of(C_, c.P, c.H, c.W, c.fout, torch.zeros(c.H, c.W, device="cuda"))
    assert all(not zero[k].any() for k in NAMES)


def test_cross_checks_on_the_device(C_):
    c = case(C_, "A")
    R, _, radii, geom, binning, img = c.fout
    got = scores_of(C_, c.P, c.H, c.W, c.fout)
    s, mx, cnt = got["sum"], got["max"], got["count"]
    # the workaround this call replaces: the feature backward of one all-ones channel under an all-ones gradient
    fb = C_.feature_maps_backward(c.P, R, c.H, c.W, geom, binning, img, None, None, 1.0, 1.0, None, None, 1.0, None, None, radii,
                                  torch.ones(c.P, 1, device="cuda"), torch.ones(1, c.H, c.W, device="cuda"), want=("features",))
    err = ((s - fb["features"][:, 0].double()).abs() / cnt.clamp(min=1)).max().item()
    print(f"[importance A] sum against the feature backward: err / max(1, count) {err:.3e} (bar 1e-5)")
    assert err <= 1e-5
    alpha = C_.aux_maps(c.P, R, c.H, c.W, geom, binning, img, maps=("alpha",))["alpha"].double().sum().item()
    total = s.sum().item()
    print(f"[importance A] sum over Gaussians {total:.6f}, the alpha map's total {alpha:.6f}")
    assert abs(total - alpha) <= 1e-5 * int(cnt.sum())   # every blended pair's weight to the value bar
    assert abs(total - alpha) <= 1e-4 * alpha
    assert float(mx.max()) <= float(np.float32(0.99))   # the forward's clamp, min(0.99f, .), times T <= 1
    assert torch.equal(cnt == 0, s == 0) and torch.equal(cnt == 0, mx == 0)
    assert (radii == 0).any() and not cnt[radii == 0].any()


def test_every_forward_path_leaves_the_same_scores(C_):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    scaling, rotation = dev(np.log(g["scales"]).astype(np.float32)), dev(g["rotations"])
    scales, rotations = C_.activate_params(scaling, rotation)
    args = forward_args(g, cam, H, W, scales, rotations)
    m = dev(random_weight(H, W, 12))
    exact = C_._forward_common(None, *args, exact=True)
    want = scores_of(C_, P, H, W, exact, m)
    assert int(want["count"].sum()) > 1000
    reserve = int(exact[0].pairs * 1.25) + 4096
    for _ in range(2):   # the reserved (graph) path, twice: the second pass of a shape is the replayed one
        reserved = C_._forward_common(None, *args, exact=False, _reserve=reserve)
        assert reserved[0].ticket > 0, "the reserved path was not taken"
        same_scores(scores_of(C_, P, H, W, reserved, m), want, "reserved")
    C_.hint_next_forward(False)   # a lean geometry blob (a forward no backward will follow)
    lean = C_._forward_common(None, *args, exact=True)
    C_.hint_next_forward(True)
    full = C_._forward_common(None, *args, exact=True)
    assert lean[3].numel() < full[3].numel(), "the hint did not select the lean blob"
    same_scores(scores_of(C_, P, H, W, lean, m), want, "lean")
    same_scores(scores_of(C_, P, H, W, full, m), want, "full")
    sh = dev(g["sh"])
    params = C_.rasterize_gaussian_params(args[0], args[1], sh[:, :1].contiguous(), sh[:, 1:].contiguous(), args[15], args[3],
                                          scaling, rotation, 1.0, args[8], args[9], cam.tanfovx, cam.tanfovy, H, W, args[16],
                                          False, False, exact=True)
    same_scores(scores_of(C_, P, H, W, params, m), want, "raw parameters")
    was = C_.set_binding("ctypes")   # the ctypes binding against the compiled one
    try:
        assert C_.binding() == "ctypes"
        plain = scores_of(C_, P, H, W, exact, m, checks=True)
    finally:
        C_.set_binding(was)
    assert C_.binding() == "torch"
    same_scores(plain, want, "ctypes binding")
    compiled = scores_of(C_, P, H, W, exact, m, checks=True)
    assert torch.equal(plain["T_check"], compiled["T_check"]) and torch.equal(plain["n_check"], compiled["n_check"])


def test_ragged_and_quantised_forwards_leave_the_same_scores(C_, golden_dir):
    from r3dgs_quantised import QuantisedModel
    from tests import test_quantised_gpu as tq
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    inputs = tq.ragged_inputs(C_, qm)
    c = tq.camera("131x77", T=(0.1, -0.05, 4.0))
    want = scores_of(C_, qm.P, c.H, c.W, tq.ragged_forward(C_, qm, inputs, c))
    assert int(want["count"].sum()) > 1000 and float(want["max"].max()) > 0.3
    same_scores(scores_of(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c)), want, "quantised")
    reserve = int(tq.ragged_forward(C_, qm, inputs, c)[0].pairs * 1.25) + 4096
    same_scores(scores_of(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c, exact=False, reserve=reserve)), want,
                "quantised, reserved")


def test_accumulation_over_three_cameras(C_):
    """accumulate=True over three views equals the single-view results folded on the host in the same order: sum bit for bit
    (one double add per view), max, count and views exactly; accumulate=False overwrites garbage and NaN."""
    kw = ar.SCENE_B
    P, H, W = kw["P"], kw["H"], kw["W"]
    singles, total = [], None
    for k, cam_seed in enumerate((5, 6, 7)):
        cam, g, _ = ar.make_scene(dict(kw, cam_seed=cam_seed))
        fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
        m = dev(random_weight(H, W, 30 + k))
        singles.append({k_: v.cpu().numpy() for k_, v in scores_of(C_, P, H, W, fout, m).items()})
        if total is None:   # the first view overwrites buffers full of garbage
            total = dict(sum=torch.full((P,), float("nan"), dtype=torch.float64, device="cuda"),
                         max=torch.full((P,), float("nan"), device="cuda"),
                         count=torch.full((P,), -12345, dtype=torch.int64, device="cuda"),
                         views=torch.full((P,), 99, dtype=torch.int32, device="cuda"))
            scores_of(C_, P, H, W, fout, m, out=total, accumulate=False)
        else:
            scores_of(C_, P, H, W, fout, m, out=total, accumulate=True)
    s = np.zeros(P)
    for one in singles:
        s = s + one["sum"]
    assert (total["sum"].cpu().numpy().view(np.uint64) == s.view(np.uint64)).all()
    assert (total["max"].cpu().numpy() == np.maximum.reduce([one["max"] for one in singles])).all()
    assert (total["count"].cpu().numpy() == sum(one["count"] for one in singles)).all()
    views = sum((one["count"] > 0).astype(np.int32) for one in singles)
    assert (total["views"].cpu().numpy() == views).all() and views.max() == 3 and ((views > 0) & (views < 3)).any()


def test_determinism_and_the_blobs_are_left_as_the_backward_needs_them(C_):
    import synth_scene as ss
    c = case(C_, "A")
    m = dev(random_weight(c.H, c.W, 13))
    same_scores(scores_of(C_, c.P, c.H, c.W, c.fout, m), scores_of(C_, c.P, c.H, c.W, c.fout, m), "two calls")
    args = forward_args(c.g, c.cam, c.H, c.W)
    dl = dev(ss.upstream_grad(c.W, c.H, seed=3) * (c.W * c.H))
    (bg, m3, colors, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args

    def grads(with_scores):
        C_.hint_next_forward(True)
        fout = C_._forward_common(None, *args, exact=True)
        if with_scores:
            scores_of(C_, c.P, c.H, c.W, fout, m)
        R, _, radii, geom, binning, img = fout
        return C_.rasterize_gaussians_backward(bg, m3, radii, colors, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom,
                                               R, binning, img, 0.0, False)
    plain, after = grads(False), grads(True)
    for k, (a, b) in enumerate(zip(plain, after)):
        assert torch.equal(a, b), k
    assert float(plain[3].abs().max()) > 0


def test_empty_model_all_culled_and_each_output_alone(C_):
    H, W = 40, 56
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=64, W=W, H=H))
    empty = {k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()}
    fout = C_._forward_common(None, *forward_args(empty, cam, H, W), exact=True)
    got = scores_of(C_, 0, H, W, fout, checks=True)
    assert all(got[k].numel() == 0 and got[k].is_cuda for k in NAMES)
    assert (got["T_check"] == 1.0).all() and not got["n_check"].any()
    behind = dict(g)
    behind["means3D"] = g["means3D"].copy()
    behind["means3D"][:, 2] = -np.abs(g["means3D"][:, 2]) - 1.0   # behind the camera: all culled
    fout = C_._forward_common(None, *forward_args(behind, cam, H, W), exact=True)
    assert int(fout[0]) == 0 and not fout[2].any()
    for binding in ("torch", "ctypes"):
        was = C_.set_binding(binding)
        try:
            got = scores_of(C_, 64, H, W, fout, checks=True)
            assert all(not got[k].any() for k in NAMES), binding
            assert (got["T_check"] == 1.0).all() and not got["n_check"].any()
            held = dict(sum=torch.full((64,), 2.5, dtype=torch.float64, device="cuda"), max=torch.full((64,), 0.25, device="cuda"),
                        count=torch.full((64,), 7, dtype=torch.int64, device="cuda"),
                        views=torch.full((64,), 3, dtype=torch.int32, device="cuda"))
            before = {k: v.clone() for k, v in held.items()}
            scores_of(C_, 64, H, W, fout, out=held, accumulate=True)   # nothing seen: the buffers keep what they held
            same_scores(held, before, binding)
            scores_of(C_, 64, H, W, fout, out=held, accumulate=False)
            assert all(not held[k].any() for k in NAMES), binding
        finally:
            C_.set_binding(was)
    # each output alone, the others NULL, under both bindings
    c = case(C_, "B")
    want = scores_of(C_, c.P, c.H, c.W, c.fout)
    for binding in ("torch", "ctypes"):
        was = C_.set_binding(binding)
        try:
            for k in NAMES:
                one = {k: torch.empty_like(want[k])}
                res = scores_of(C_, c.P, c.H, c.W, c.fout, out=one)
                assert set(res) == {k} and torch.equal(one[k], want[k]), (binding, k)
        finally:
            C_.set_binding(was)
    for bad in (dict(sum=want["sum"].float()), dict(max=want["max"][:-1]), dict(count=torch.empty(c.P, 2, dtype=torch.int64, device="cuda")[:, 0]),
                dict(views=want["views"].cpu())):
        with pytest.raises((RuntimeError, ValueError)):
            scores_of(C_, c.P, c.H, c.W, c.fout, out=bad)
    with pytest.raises(RuntimeError, match="float32"):
        scores_of(C_, c.P, c.H, c.W, c.fout, torch.ones(c.H, c.W, dtype=torch.float64, device="cuda"))


def test_captured_launch_replays_over_fixed_buffers(C_):
    """Only the scoring call is captured, over fixed state buffers, a fixed weight map and fixed outputs; replayed after two
    different forwards whose blobs were copied into those buffers, each replay equals the direct call on the forward's own
    blobs, under the other binding as well."""
    kw = ar.SCENE_A
    P, H, W = kw["P"], kw["H"], kw["W"]
    passes = []
    for gseed in (kw["gseed"], kw["gseed"] + 1):
        cam, g, _ = ar.make_scene(dict(kw, gseed=gseed))
        args = forward_args(g, cam, H, W)
        reserve = 3 * int(C_._forward_common(None, *args, exact=True)[0].pairs) + 4096 if not passes else passes[0][0].capacity
        fout = C_._forward_common(None, *args, exact=False, _reserve=reserve)
        assert fout[0].ticket > 0 and not fout[0].truncated
        passes.append(fout)
    first, second = passes
    fixed = [torch.empty_like(t) for t in first[3:]]
    for dst, src in zip(fixed, first[3:]):
        dst.copy_(src)
    m = dev(random_weight(H, W, 14))
    static = {k: torch.empty(P, dtype=C_._SCORE_DTYPES[k], device="cuda") for k in NAMES}
    call = lambda blobs, out=None: C_.contribution_scores(P, first[0], H, W, *blobs, pixel_weight=m, out=out)   # noqa: E731
    call(fixed, static)   # warm-up outside the capture (the workspace size is asked here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(fixed, static)
    for fout in (first, second, first):
        for dst, src in zip(fixed, fout[3:]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want = call(list(fout[3:]))
        same_scores({k: v.clone() for k, v in static.items()}, want, "replay")
        was = C_.set_binding("ctypes")
        try:
            same_scores(call(list(fout[3:])), want, "ctypes binding")
        finally:
            C_.set_binding(was)
    assert not torch.equal(call(list(first[3:]))["sum"], call(list(second[3:]))["sum"])


def _model_and_views(n_views):
    from tests import test_densify_gpu as td
    kw = ar.SCENE_A
    P, H, W = kw["P"], kw["H"], kw["W"]
    views, g = [], None
    for k in range(n_views):
        cam, g, _ = ar.make_scene(dict(kw, cam_seed=kw["cam_seed"] + k))
        views.append(NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
                        full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center)))
    state = dict(xyz=g["means3D"], f_dc=g["sh"][:, :1], f_rest=g["sh"][:, 1:], opacity=g["opacity"].reshape(P, 1),
                 scaling=np.log(g["scales"]).astype(np.float32), rotation=g["rotations"], degrees=g["degrees"],
                 xyz_gradient_accum=np.zeros((P, 1), np.float32), denom=np.zeros((P, 1), np.float32),
                 max_radii2D=np.zeros(P, np.float32))
    return td._model(state), views, NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False), P, H, W


def test_camera_set_module(C_):
    """r3dgs_importance over four cameras without a host wait, the mask, and prune_points on it."""
    import r3dgs_densify
    import r3dgs_importance as ri
    pc, views, pipe, P, H, W = _model_and_views(4)
    bg = dev(BG)
    weights = [dev(random_weight(H, W, 40 + k)).abs() for k in range(4)]
    ri.contribution_scores(views[:1], pc, pipe, bg)   # warm-up: the first pass of a shape asks sizes
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total = ri.contribution_scores(views, pc, pipe, bg, pixel_weights=weights)
        seen = []
        by_callable = ri.contribution_scores(views, pc, pipe, bg,
                                             pixel_weights=lambda i, cam, pkg: (seen.append((i, tuple(pkg["render"].shape))), weights[i])[1])
        mask = ri.low_contribution_mask(total, keep_fraction=0.5)
        lenient = ri.low_contribution_mask(total, max_below=0.05, never_seen=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert seen == [(i, (3, H, W)) for i in range(4)]
    same_scores(total._asdict(), by_callable._asdict(), "sequence against callable")
    fold = None
    for v, m in zip(views, weights):
        one = ri.view_scores(v, pc, pipe, bg, pixel_weight=m)
        fold = one if fold is None else ri.Scores(fold.sum + one.sum, torch.maximum(fold.max, one.max), fold.count + one.count,
                                                  fold.views + one.views)
    same_scores(total._asdict(), fold._asdict(), "the loop against view_scores folded in torch")
    assert int(total.views.max()) == 4 and bool((total.count == 0).any())
    unseen = total.count == 0
    assert bool(mask[unseen].all()) and not bool(lenient[unseen].any())
    assert bool((lenient == ((total.max < 0.05) & ~unseen)).all()) and bool(lenient.any())
    keep = ~mask
    assert int(keep.sum()) <= (P + 1) // 2 and int(keep.sum()) > 0
    assert float(total.sum[keep].min()) >= float(total.sum[mask & ~unseen].max())
    kept_xyz = pc._xyz.detach()[keep].clone()
    r3dgs_densify.prune_points(pc, mask)
    assert torch.equal(pc._xyz.detach(), kept_xyz) and pc._opacity.shape[0] == int(keep.sum())
    # refusals come before any launch
    with pytest.raises(ValueError, match="pixel_weight"):
        ri.contribution_scores(views, pc, pipe, bg, pixel_weights=[torch.ones(H, W + 1, device="cuda")] * 4)
    with pytest.raises(ValueError, match="4 cameras"):
        ri.contribution_scores(views, pc, pipe, bg, pixel_weights=weights[:2])
    with pytest.raises(ValueError, match="no cameras"):
        ri.contribution_scores([], pc, pipe, bg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ri.view_scores(views[0], pc, pipe, bg.cpu())
    with pytest.raises(ValueError, match="float32"):
        ri.view_scores(views[0], pc, pipe, bg, pixel_weight=torch.ones(H, W, dtype=torch.float64, device="cuda"))


def test_camera_set_module_with_a_quantised_model(C_):
    import r3dgs_importance as ri
    from tests import test_quantised_gpu as tq
    qm, _ = tq.model("37-0-150-70")
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    views = []
    for T in ((0.0, 0.0, 4.0), (0.1, -0.05, 4.0)):
        c = tq.camera("131x77", T=T)
        views.append((c, NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm,
                            full_proj_transform=c.pm, camera_center=c.cp)))
    total = ri.contribution_scores([v for _, v in views], qm, pipe, views[0][0].bg)
    s = torch.zeros(qm.P, dtype=torch.float64, device="cuda")
    for c, _ in views:
        s = s + scores_of(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c))["sum"]
    assert torch.equal(total.sum, s) and int(total.views.max()) == 2 and float(total.max.max()) > 0.3
