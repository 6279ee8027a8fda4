"""GPU tests (-m gpu) of the feature maps (include/r3dgs_features.h, csrc/feature_maps.hip): a per-Gaussian feature vector
blended into a [C,H,W] map and the gradients through it -- against the float64 reference tests/feature_ref.py, against the
library's own colour render / colour backward over a black background and its depth map, after every forward entry point, with
NULL outputs, for determinism and untouched state, inside a captured graph, at the edges and through r3dgs_render.render.

Bars (the project's own): values within 1e-5 * max(1, max |F|); gradients max |got - ref| <= 1e-4 * max |ref| per tensor.  Both
off the oracle's threshold-ambiguous pixels (at most 0.1 %, asserted by the shared Case), which carry a zero upstream gradient
on both sides."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import aux_ref as ar
from tests import camera_cases as cc
from tests import feature_ref as fr
from tests import test_aux_grad_gpu as tg
from tests.test_aux_grad_gpu import EMPTY, Case, Model, dev, forward_args

pytestmark = pytest.mark.gpu
REL = 1e-4
GROUP = 16   # feature_math.h kFeatGroup
CHANNELS = (1, 3, GROUP, GROUP + 1, 2 * GROUP + 3)
GEOM = ("means2D", "means3D", "opacity", "scales", "rotations")


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


def features_of(P, C, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (P, C)).astype(np.float32)


def upstream(c, C, seed=2):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (C, c.H * c.W)).astype(np.float32) * c.ok[None, :]


def fwd(C_, c, F, fout=None):
    R, _, _, geom, binning, img = c.fout if fout is None else fout
    return C_.feature_maps(c.P, R, c.H, c.W, geom, binning, img, F if isinstance(F, torch.Tensor) else dev(F))


def bwd(C_, c, F, g, want=None, fout=None, g_=None):
    R, _, radii, geom, binning, img = c.fout if fout is None else fout
    cam, m = c.cam, c.g
    return C_.feature_maps_backward(c.P, R, c.H, c.W, geom, binning, img, dev(cam.world_view_transform), dev(cam.full_proj_transform),
                                    cam.tanfovx, cam.tanfovy, dev(m["means3D"]), dev(m["scales"]), 1.0, dev(m["rotations"]), EMPTY,
                                    radii, F if isinstance(F, torch.Tensor) else dev(F), g if isinstance(g, torch.Tensor) else dev(g),
                                    **({} if want is None else {"want": want}))


def reference(c, C):
    """feature_ref's map and gradients for the case's seeded F and g at C channels: computed once, shared, never modified."""
    cache = c.__dict__.setdefault("_feature_refs", {})
    if C not in cache:
        F, g = features_of(c.P, C), upstream(c, C)
        m, cam = c.g, c.cam
        cache[C] = (F, g, fr.reference_grads(c.st, m["means3D"], m["opacity"], m["scales"], m["rotations"], cam.world_view_transform,
                                             cam.full_proj_transform, cam.tanfovx, cam.tanfovy, F, g))
    return cache[C]


def held(got, ref, names, what):
    for k in names:
        a, b = got[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        if k == "means2D":
            assert not a[:, 2].any()
            a = a[:, :2]
        scale, err = np.abs(b).max(), np.abs(a - b.reshape(a.shape)).max()
        print(f"[feature maps {what}] {k}: max err {err:.3e}, bar {REL * scale:.3e} (max |ref| {scale:.3e})")
        assert scale > 0 and err <= REL * scale, (what, k, err, scale)


def value_held(got, want, ok, fmax, what):
    err = np.abs(got.reshape(want.shape) - want)[:, ok].max()
    bar = 1e-5 * max(1.0, fmax)
    print(f"[feature maps {what}] value error {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (what, err)


@pytest.fixture(scope="module")
def scene_a(C_):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    ex = C_.export_binning(c.P, c.fout[0], c.H, c.W, c.fout[3], c.fout[4], c.fout[5])
    lens = (ex["ranges"][:, 1] - ex["ranges"][:, 0]).cpu().numpy()
    print(f"[feature maps scene A] heaviest tile list {lens.max()} entries")
    assert lens.max() > 128, "scene A must have a list of two full staging chunks and a remainder"
    return c


@pytest.fixture(scope="module")
def scene_b(C_):
    kw = ar.SCENE_B
    cam, g, _ = ar.make_scene(kw)
    return Case(C_, cam, g, kw["H"], kw["W"])


@pytest.fixture(scope="module")
def portrait(C_):
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", 600, ar.PORTRAIT["seed"])
    return Case(C_, cam, g, cam.image_height, cam.image_width)


def pick(name, scene_a, scene_b, portrait):
    return dict(A=scene_a, B=scene_b, portrait=portrait)[name]


@pytest.mark.parametrize("name,C", [("A", C) for C in CHANNELS] + [("B", GROUP + 1), ("portrait", GROUP + 1)])
def test_forward_parity(C_, scene_a, scene_b, portrait, name, C):
    c = pick(name, scene_a, scene_b, portrait)
    F = features_of(c.P, C)
    got = fwd(C_, c, F)
    assert got.shape == (C, c.H, c.W) and got.dtype == torch.float32 and not got.requires_grad
    # the reference's map over the state's own fp32 means and conics -- the numbers the kernel reads -- in float64
    value_held(got.cpu().numpy(), fr.feature_map(c.st, F), c.ok.astype(bool), float(np.abs(F).max()), f"scene {name}, C = {C}")
    empty = (np.asarray(c.st["n_contrib"]).reshape(-1) == 0) & c.ok.astype(bool)
    assert not got.reshape(C, -1).cpu().numpy()[:, empty].any()


def test_forward_against_the_library_itself(C_, scene_a):
    """Channels 3i..3i+2 are the image of a colors_precomp render over a black background; the channel F = z is the depth map."""
    c = scene_a
    V = np.asarray(c.cam.world_view_transform, np.float64).reshape(4, 4)
    z = (np.concatenate([c.g["means3D"], np.ones((c.P, 1), np.float32)], 1).astype(np.float64) @ V)[:, 2].astype(np.float32)
    F = np.abs(features_of(c.P, 7, 3))
    F[:, 6] = z
    got = fwd(C_, c, F).cpu().numpy()
    ok = c.ok.astype(bool).reshape(c.H, c.W)
    for i in range(2):
        out = C_._forward_common(None, *forward_args(c.g, c.cam, c.H, c.W, colors=dev(np.ascontiguousarray(F[:, 3 * i:3 * i + 3]))), exact=True)
        err = np.abs(got[3 * i:3 * i + 3] - out[1].cpu().numpy())[:, ok].max()
        print(f"[feature maps] channels {3 * i}..{3 * i + 2} against the colour render: {err:.3e}")
        assert err <= 1e-5
    R, _, _, geom, binning, img = c.fout
    depth = C_.aux_maps(c.P, R, c.H, c.W, geom, binning, img, maps=("depth",))["depth"][0].cpu().numpy()
    err = np.abs(got[6] - depth)[ok].max()
    print(f"[feature maps] F = z against the depth map: {err:.3e} (bar {1e-5 * max(1.0, float(z.max())):.3e})")
    assert err <= 1e-5 * max(1.0, float(np.abs(F).max()))


def test_every_forward_entry_point_leaves_the_same_map(C_, golden_dir):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    F = dev(features_of(P, GROUP + 1, 4))
    scaling, rotation = dev(np.log(g["scales"]).astype(np.float32)), dev(g["rotations"])
    scales, rotations = C_.activate_params(scaling, rotation)
    from tests.test_aux_maps_gpu import forward_args as fa
    args = fa(g, cam, H, W, scales, rotations)
    exact = C_._forward_common(None, *args, exact=True)
    of = lambda fout: C_.feature_maps(P, fout[0], H, W, fout[3], fout[4], fout[5], F)   # noqa: E731
    want = of(exact)
    assert float(want.abs().max()) > 0.1
    reserve = int(exact[0].pairs * 1.25) + 4096
    for _ in range(2):   # the second pass of a shape is the replayed one
        reserved = C_._forward_common(None, *args, exact=False, _reserve=reserve)
        assert reserved[0].ticket > 0, "the reserved path was not taken"
        assert torch.equal(of(reserved), want), "reserved"
    C_.hint_next_forward(False)
    lean = C_._forward_common(None, *args, exact=True)
    assert torch.equal(of(lean), want), "lean"
    sh = dev(g["sh"])
    params = C_.rasterize_gaussian_params(args[0], args[1], sh[:, :1].contiguous(), sh[:, 1:].contiguous(), args[15], args[3],
                                          scaling, rotation, 1.0, args[8], args[9], cam.tanfovx, cam.tanfovy, H, W, args[16],
                                          False, False, exact=True)
    assert torch.equal(of(params), want), "raw parameters"
    # the quantised forward of the tests/golden P200 model against the ragged inference forward of its decoded model
    from r3dgs_quantised import QuantisedModel
    from tests import test_quantised_gpu as tq
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    c = tq.camera("131x77", T=(0.1, -0.05, 4.0))
    Fq = dev(features_of(qm.P, GROUP + 1, 5))
    ragged = tq.ragged_forward(C_, qm, tq.ragged_inputs(C_, qm), c)
    quant = tq.quantised_forward(C_, qm, c)
    a = C_.feature_maps(qm.P, ragged[0], c.H, c.W, ragged[3], ragged[4], ragged[5], Fq)
    b = C_.feature_maps(qm.P, quant[0], c.H, c.W, quant[3], quant[4], quant[5], Fq)
    assert float(a.abs().max()) > 0.1 and torch.equal(a, b), "quantised"


@pytest.mark.parametrize("name,C", [("A", 3), ("A", GROUP + 1), ("A", 2 * GROUP + 3), ("B", GROUP + 1), ("portrait", GROUP + 1)])
def test_backward_parity(C_, scene_a, scene_b, portrait, name, C):
    c = pick(name, scene_a, scene_b, portrait)
    F, g, ref = reference(c, C)
    was = C_.set_f64_chain(True)
    try:
        for f64 in (True, False):
            C_.set_f64_chain(f64)
            got = bwd(C_, c, F, g)
            assert got["features"].shape == (c.P, C)
            held(got, ref, ("features",) + GEOM, f"scene {name}, C = {C}, f64_chain={f64}")
    finally:
        C_.set_f64_chain(was)


@pytest.mark.parametrize("name,channels", [("P65_17x19", (1, 4, 5, 8, 9, GROUP, GROUP + 1)), ("P1_17x19", (5,))])
def test_small_models_on_a_17x19_image(C_, name, channels):
    """P = 65 (one Gaussian past a wave) and P = 1 on 17x19, partial tiles on both axes: map and every gradient against the
    reference.  On the P = 65 scene the backward runs at every channel count around its group widths (4, 8, 16): one short of a
    full group, full, and one past it."""
    kw = ar.SMALL[name]
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    for C in channels:
        F, up, ref = reference(c, C)
        value_held(fwd(C_, c, F).cpu().numpy(), fr.feature_map(c.st, F), c.ok.astype(bool), 1.0, f"{name}, C = {C}")
        got = bwd(C_, c, F, up)
        assert got["features"].shape == (c.P, C)
        held(got, ref, ("features",) + GEOM, f"{name}, C = {C}")


def test_backward_with_a_precomputed_covariance(C_, scene_b):
    c = scene_b
    g, cam, C = c.g, c.cam, 3
    q, S = g["rotations"].astype(np.float64), g["scales"].astype(np.float64)
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = Rm * S[:, None, :]
    Sig = L @ L.transpose(0, 2, 1)
    cov = np.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1).astype(np.float32)
    args = list(forward_args(g, cam, c.H, c.W))
    args[4], args[5], args[7] = EMPTY, EMPTY, dev(cov)
    fout = C_._forward_common(None, *args, exact=True)
    assert torch.equal(fout[2] > 0, c.fout[2] > 0), "the two forwards must see the same splats"
    F, up = features_of(c.P, C, 6), upstream(c, C, 7)
    R, _, radii, geom, binning, img = fout
    got = C_.feature_maps_backward(c.P, R, c.H, c.W, geom, binning, img, dev(cam.world_view_transform), dev(cam.full_proj_transform),
                                   cam.tanfovx, cam.tanfovy, dev(g["means3D"]), EMPTY, 1.0, EMPTY, dev(cov), radii, dev(F), dev(up))
    ref = fr.reference_grads(c.st, g["means3D"], g["opacity"], None, None, cam.world_view_transform, cam.full_proj_transform,
                             cam.tanfovx, cam.tanfovy, F, up, cov3D_precomp=cov)
    assert not got["scales"].any() and not got["rotations"].any()
    held(got, ref, ("features", "means2D", "means3D", "opacity", "cov3D"), "cov3D_precomp")


def test_backward_against_the_colour_backward(C_, scene_a):
    """C = 7 zero-padded to 9: grad_colors_precomp of the three black-background renders, concatenated, is dL_dfeatures, and the
    sum of their geometry gradients is this call's."""
    c = scene_a
    g, cam, H, W, C = c.g, c.cam, c.H, c.W, 7
    F = np.zeros((c.P, 9), np.float32)
    F[:, :C] = np.abs(features_of(c.P, C, 8))
    up = np.zeros((9, H * W), np.float32)
    up[:C] = upstream(c, C, 9)
    new = bwd(C_, c, F[:, :C], up[:C])
    total = None
    dcols = []
    for i in range(3):
        col = dev(np.ascontiguousarray(F[:, 3 * i:3 * i + 3]))
        args = forward_args(g, cam, H, W, colors=col)
        C_.hint_next_forward(True)
        fout = C_._forward_common(None, *args, exact=True)
        (bg, m3, _, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
        R, _, radii, geom, binning, img = fout
        old = C_.rasterize_gaussians_backward(bg, m3, radii, col, sc, rot, mod, cov, vm, pm, tx, ty, dev(up[3 * i:3 * i + 3].reshape(3, H, W)),
                                              sh, deg, campos, geom, R, binning, img, 0.0, False)
        m2, dcol, dop, dm3, _, _, dsc, drot = [t.cpu().numpy().astype(np.float64) for t in old]
        dcols.append(dcol)
        part = dict(means2D=m2[:, :2], opacity=dop, scales=dsc, rotations=drot, means3D=dm3)
        total = part if total is None else {k: total[k] + part[k] for k in part}
    total["features"] = np.concatenate(dcols, 1)[:, :C]
    held(new, total, ("features",) + GEOM, "against the colour backward")


def test_null_outputs_equal_the_full_call(C_, scene_a):
    c = scene_a
    F, g, _ = reference(c, GROUP + 1)
    full = bwd(C_, c, F, g, want=C_.FEATURE_GRADS)
    assert float(full["cov3D"].abs().max()) > 0
    only_f = bwd(C_, c, F, g, want=("features",))
    assert set(only_f) == {"features"} and torch.equal(only_f["features"], full["features"])
    only_g = bwd(C_, c, F, g, want=C_.AUX_GRADS)
    assert set(only_g) == set(C_.AUX_GRADS)
    for k in C_.AUX_GRADS:
        assert torch.equal(only_g[k], full[k]), k
    one = bwd(C_, c, F, g, want=("opacity",))
    assert torch.equal(one["opacity"], full["opacity"])
    assert bwd(C_, c, F, g, want=()) == {}   # no output asked for: nothing comes back
    none = bwd(C_, c, F, None, want=C_.FEATURE_GRADS)
    assert all(not t.any() for t in none.values())
    # frozen geometry needs none of the camera and geometry inputs
    R, _, radii, geom, binning, img = c.fout
    bare = C_.feature_maps_backward(c.P, R, c.H, c.W, geom, binning, img, None, None, 1.0, 1.0, None, None, 1.0, None, None, radii,
                                    dev(F), dev(g), want=("features",))
    assert torch.equal(bare["features"], full["features"])


def test_determinism_and_untouched_state(C_, scene_a):
    import synth_scene as ss
    c = scene_a
    g, cam, H, W = c.g, c.cam, c.H, c.W
    F, up, _ = reference(c, 2 * GROUP + 3)
    args = forward_args(g, cam, H, W)
    (bg, m3, colors, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
    dl = dev(ss.upstream_grad(W, H, seed=3) * (W * H))

    def run(with_features):
        C_.hint_next_forward(True)
        fout = C_._forward_common(None, *args, exact=True)
        R, _, radii, geom, binning, img = fout
        if with_features:
            before = [t.clone() for t in (geom, binning, img)]
            a, b = fwd(C_, c, F, fout), fwd(C_, c, F, fout)
            assert torch.equal(a, b)
            x, y = bwd(C_, c, F, up, C_.FEATURE_GRADS, fout), bwd(C_, c, F, up, C_.FEATURE_GRADS, fout)
            for k in x:
                assert torch.equal(x[k], y[k]), k
            for p, q in zip(before, (geom, binning, img)):
                assert torch.equal(p, q), "a state blob was written"
        return C_.rasterize_gaussians_backward(bg, m3, radii, colors, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom,
                                               R, binning, img, 0.0, False)
    for k, (a, b) in enumerate(zip(run(False), run(True))):
        assert torch.equal(a, b), k


def test_captured_launches_follow_their_buffers(C_, scene_a):
    c = scene_a
    C = GROUP + 1
    first, second = (features_of(c.P, C, 11), upstream(c, C, 12)), (features_of(c.P, C, 13), upstream(c, C, 14))
    F, g = dev(first[0]), dev(first[1])

    R, _, radii, geom, binning, img = c.fout
    fixed = [dev(a) for a in (c.cam.world_view_transform, c.cam.full_proj_transform, c.g["means3D"], c.g["scales"], c.g["rotations"])]

    def go():   # (every input already on the device: nothing but the library's launches is captured)
        return (C_.feature_maps(c.P, R, c.H, c.W, geom, binning, img, F),
                C_.feature_maps_backward(c.P, R, c.H, c.W, geom, binning, img, fixed[0], fixed[1], c.cam.tanfovx, c.cam.tanfovy,
                                         fixed[2], fixed[3], 1.0, fixed[4], EMPTY, radii, F, g))
    go()   # warm-up outside the capture (the workspace size is asked here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        smap, sgrad = go()
    for Fn, gn in (second, first):
        F.copy_(dev(Fn))
        g.copy_(dev(gn))
        graph.replay()
        torch.cuda.synchronize()
        dmap, dgrad = fwd(C_, c, Fn), bwd(C_, c, Fn, gn)
        assert torch.equal(smap, dmap)
        for k in dgrad:
            assert torch.equal(sgrad[k], dgrad[k]), k
    assert not torch.equal(fwd(C_, c, second[0]), smap)


def test_edges(C_):
    H, W = 40, 56
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=64, W=W, H=H))
    C = GROUP + 1
    view = (dev(cam.world_view_transform), dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy)

    def both(model, fout, F, up):
        R, _, radii, geom, binning, img = fout
        P = len(model["means3D"])
        m = C_.feature_maps(P, R, H, W, geom, binning, img, F)
        d = C_.feature_maps_backward(P, R, H, W, geom, binning, img, *view, dev(model["means3D"]), dev(model["scales"]), 1.0,
                                     dev(model["rotations"]), EMPTY, radii, F, up)
        return m, d
    up = torch.ones(C, H, W, device="cuda")
    empty = {k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()}
    m, d = both(empty, C_._forward_common(None, *forward_args(empty, cam, H, W), exact=True), torch.zeros(0, C, device="cuda"), up)
    assert m.shape == (C, H, W) and not m.any() and all(t.shape[0] == 0 for t in d.values())
    behind = dict(g)
    behind["means3D"] = g["means3D"].copy()
    behind["means3D"][:, 2] = -np.abs(g["means3D"][:, 2]) - 1.0
    fout = C_._forward_common(None, *forward_args(behind, cam, H, W), exact=True)
    assert int(fout[0]) == 0 and not fout[2].any()   # every Gaussian culled: R = 0
    m, d = both(behind, fout, dev(features_of(64, C)), up)
    assert not m.any() and all(t.shape[0] == 64 and not t.any() for t in d.values())
    F = dev(features_of(64, C))
    fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
    R, _, radii, geom, binning, img = fout
    for bad in (torch.zeros(64, 0, device="cuda"), torch.zeros(64, C_.FEATURE_MAX_CHANNELS + 1, device="cuda")):
        with pytest.raises(ValueError, match="C ="):
            C_.feature_maps(64, R, H, W, geom, binning, img, bad)
    assert C_._lib.r3dgs_feature_maps(64, 16, W, H, geom.data_ptr(), binning.data_ptr(), img.data_ptr(), F.data_ptr(), 0, None, None) < 0


def test_one_partial_tile(C_):
    """A 5x3 image: one tile, three of its quadrants empty of pixels."""
    kw = dict(ar.SCENE_17, W=5, H=3, f=4.0)
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, 3, 5)
    F, up, ref = reference(c, GROUP + 1)
    value_held(fwd(C_, c, F).cpu().numpy(), fr.feature_map(c.st, F), c.ok.astype(bool), 1.0, "5x3")
    assert np.abs(ref["map"]).max() > 0.01
    held(bwd(C_, c, F, up), ref, ("features",) + GEOM, "5x3")


def test_overflowed_reservation(C_, scene_a):
    """Half the pairs reserved, strict mode off: the Gaussians that lost pairs get zero rows; every other row is what the colour
    backward gives over the same truncated state (C = 3, colours F over black)."""
    c = scene_a
    g, cam, H, W = c.g, c.cam, c.H, c.W
    F = np.abs(features_of(c.P, 3, 15))
    up = upstream(c, 3, 16)
    col = dev(F)
    args = forward_args(g, cam, H, W, colors=col)
    (bg, m3, _, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
    exact = C_._forward_common(None, *args, exact=True)
    C_.hint_next_forward(True)
    fout = C_._forward_common(None, *args, exact=False, _reserve=exact[0].pairs // 2, _strict_override=False)
    assert bool(fout[0].truncated)
    R, _, radii, geom, binning, img = fout
    dl = dev(up.reshape(3, H, W))
    old = C_.rasterize_gaussians_backward(bg, m3, radii, col, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom, R, binning,
                                          img, 0.0, False)
    C_.hint_next_forward(True)
    fex = C_._forward_common(None, *args, exact=True)
    full = C_.rasterize_gaussians_backward(bg, m3, fex[2], col, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, fex[3], fex[0],
                                           fex[4], fex[5], 0.0, False)
    dropped = (full[0].abs().sum(dim=1) > 0) & (old[0].abs().sum(dim=1) == 0)
    assert int(dropped.sum()) > 0, "no Gaussian lost its pairs: the reservation did not overflow"
    new = bwd(C_, c, F, up, fout=fout)
    for k in ("features", "means2D", "opacity"):
        assert not new[k][dropped].any(), k
    m2, dcol, dop = [t.cpu().numpy().astype(np.float64) for t in old[:3]]
    held(new, dict(features=dcol, means2D=m2[:, :2], opacity=dop), ("features", "means2D", "opacity"), "overflowed reservation")


def view_of(cam, H, W):
    return NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))


PIPE = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def test_through_render(C_, scene_a):
    import r3dgs_render
    c = scene_a
    H, W, C = c.H, c.W, GROUP + 1
    F0, g, ref = reference(c, C)
    pc, view, bg = Model(c.g), view_of(c.cam, H, W), dev(tg.BG)
    # (Model scales its rotations by 1.3: the kernels normalise them, and so does the reference's chain below)
    plain = r3dgs_render.render(view, pc, PIPE, bg)
    none = r3dgs_render.render(view, pc, PIPE, bg, features=None)
    assert set(none) == set(plain) and torch.equal(none["render"], plain["render"]) and torch.equal(none["radii"], plain["radii"])
    wimg = dev(np.linspace(0.5, 1.5, 3 * H * W, dtype=np.float32).reshape(3, H, W))
    gmap = dev(g.reshape(C, H, W))

    def backward_of(loss_of, **kw):
        for t in pc.leaves():
            t.grad = None
        F = dev(F0).requires_grad_(True)
        out = r3dgs_render.render(view, pc, PIPE, bg, features=F, **kw)
        loss_of(out).backward()
        vs = out["viewspace_points"].grad
        return [torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in pc.leaves()] + \
               [torch.zeros_like(pc._xyz) if vs is None else vs.clone()], F.grad, out
    for t in pc.leaves():
        t.grad = None
    (plain["render"] * wimg).sum().backward()
    colour_only = [t.grad.clone() for t in pc.leaves()] + [plain["viewspace_points"].grad.clone()]
    frozen, Fgrad, out = backward_of(lambda o: (o["render"] * wimg).sum() + (o["features"] * gmap).sum())
    assert set(out) == set(plain) | {"features"} and out["features"].shape == (C, H, W) and out["features"].requires_grad
    assert torch.equal(out["render"], plain["render"])
    held(dict(features=Fgrad), ref, ("features",), "render, F.grad")
    for a, b in zip(frozen, colour_only):
        assert torch.equal(a, b), "features_geom_grad=False must leave the colour-only gradients bit for bit"
    both, Fgrad2, out2 = backward_of(lambda o: (o["render"] * wimg).sum() + (o["features"] * gmap).sum(), features_geom_grad=True,
                                     aux=("alpha",))
    assert torch.equal(Fgrad2, Fgrad) and torch.equal(out2["features"], out["features"]) and "alpha" in out2
    # feature_ref's share, chained through torch's exp / normalize by hand (aux_grad's test does the same)
    scales = torch.exp(pc._scaling).detach()
    leaf = pc._rotation.detach().clone().requires_grad_(True)
    drot, = torch.autograd.grad(torch.nn.functional.normalize(leaf), leaf, dev(ref["rotations"].astype(np.float32)))
    m2 = np.concatenate([ref["means2D"], np.zeros((c.P, 1))], 1).astype(np.float32)
    share = [dev(ref["means3D"].astype(np.float32)), None, None, dev(ref["opacity"].astype(np.float32)),
             dev(ref["scales"].astype(np.float32)) * scales, drot, dev(m2)]
    for k, (got, base, add) in enumerate(zip(both, colour_only, share)):
        if add is None:
            assert torch.equal(got, base), k
            continue
        want = base.double() + add.double()   # the reference of this tensor: the bar is 1e-4 of ITS largest entry
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        print(f"[feature maps render] model gradient {k}: colour-only + feature_ref's share, err {err:.3e} (bar {REL * scale:.3e})")
        assert float(add.abs().max()) > 0 and err <= REL * scale, (k, err, scale)
    # a non-contiguous F is made contiguous; a detached F gives a detached map
    Ft = dev(np.ascontiguousarray(F0.T)).t()
    assert not Ft.is_contiguous()
    got = r3dgs_render.render(view, pc, PIPE, bg, features=Ft)["features"]
    assert torch.equal(got, out["features"]) and not got.requires_grad
    # the refusals
    F = dev(F0)
    for bad in (F[:-1], F.double(), F.cpu(), F[:, :0], torch.zeros(c.P, C_.FEATURE_MAX_CHANNELS + 1, device="cuda"), F.reshape(-1)):
        with pytest.raises(ValueError, match="features"):
            r3dgs_render.render(view, pc, PIPE, bg, features=bad)
    with pytest.raises(ValueError, match="no_grad"), torch.no_grad():
        r3dgs_render.render(view, pc, PIPE, bg, features=F, features_geom_grad=True)
    grad_view = view_of(c.cam, H, W)
    grad_view.world_view_transform = grad_view.world_view_transform.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="camera"):
        r3dgs_render.render(grad_view, pc, PIPE, bg, features=F, features_geom_grad=True)


def test_through_render_quantised(C_, golden_dir):
    import r3dgs_render
    from r3dgs_quantised import QuantisedModel
    from tests import test_quantised_gpu as tq
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    c = tq.camera("131x77", T=(0.1, -0.05, 4.0))
    qview = NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm, full_proj_transform=c.pm,
               camera_center=c.cp)
    F = dev(features_of(qm.P, 5, 17)).requires_grad_(True)
    out = r3dgs_render.render(qview, qm, PIPE, c.bg, features=F)
    quant = tq.quantised_forward(C_, qm, c)
    assert torch.equal(out["features"], C_.feature_maps(qm.P, quant[0], c.H, c.W, quant[3], quant[4], quant[5], F))
    out["features"].sum().backward()
    want = C_.feature_maps_backward(qm.P, quant[0], c.H, c.W, quant[3], quant[4], quant[5], None, None, 1.0, 1.0, None, None, 1.0,
                                    None, None, quant[2], F, torch.ones(5, c.H, c.W, device="cuda"), want=("features",))
    assert float(F.grad.abs().max()) > 0 and torch.equal(F.grad, want["features"])
    with pytest.raises(ValueError, match="QuantisedModel"):
        r3dgs_render.render(qview, qm, PIPE, c.bg, features=F, features_geom_grad=True)


def test_adam_on_the_features_alone(C_, scene_b):
    """Forty r3dgs_optim.Adam steps on F against a fixed target map, and the same loop in float64 on feature_ref (both take
    the same decisions: fp32 rounding is all that separates them).  The GPU's loss ratio may exceed the float64 one by at most
    10 % of it."""
    import r3dgs_optim
    import r3dgs_render
    c = scene_b
    H, W, C, steps, lr = c.H, c.W, GROUP + 1, 40, 0.05
    pc, view, bg = Model(c.g), view_of(c.cam, H, W), dev(tg.BG)
    ok = c.ok.astype(bool)
    target = fr.feature_map(c.st, features_of(c.P, C, 21)) * ok[None, :]
    F0 = features_of(c.P, C, 22)
    okd, tgt = dev(c.ok.reshape(1, H, W)), dev(target.astype(np.float32).reshape(C, H, W))
    F = dev(F0).requires_grad_(True)
    opt = r3dgs_optim.Adam([F], lr=lr)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        m = r3dgs_render.render(view, pc, PIPE, bg, features=F)["features"]
        loss = (((m - tgt) * okd) ** 2).sum()
        losses.append(float(loss))
        loss.backward()
        opt.step()
    # float64: the map is linear in F -- one Jacobian-free loop on the reference's walk
    xy, co = fr._t(c.st["xy"]), fr._t(c.st["conic_op"])
    Fd = fr._t(F0).requires_grad_(True)
    optd = torch.optim.Adam([Fd], lr=lr)
    tgtd, okt = torch.from_numpy(target), torch.from_numpy(ok.astype(np.float64))[None, :]
    lossesd = []
    for _ in range(steps + 1):
        optd.zero_grad(set_to_none=True)
        loss = (((fr.walk(c.st, xy, co, Fd) - tgtd) * okt) ** 2).sum()
        lossesd.append(float(loss))
        loss.backward()
        optd.step()
    ratio, ratiod = losses[-1] / losses[0], lossesd[-1] / lossesd[0]
    print(f"[feature maps Adam] loss ratio after {steps} steps: GPU {ratio:.6f}, float64 reference {ratiod:.6f}")
    assert ratiod < 1.0 and ratio <= 1.1 * ratiod
