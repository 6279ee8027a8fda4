"""GPU tests (-m gpu) of the auxiliary maps (include/r3dgs_aux.h, csrc/aux_maps.hip): expected depth, alpha and median depth
replayed from the state a forward left, against tests/aux_ref.py over the oracle re-binned into the HIP rects, against the
forward's own final_T / n_contrib bit for bit, across every forward entry point and both bindings, with the backward after
it, at the edges, inside a captured graph and through r3dgs_render.render(aux=...).

Bars:
  * depth: |depth - ref| <= 1e-5 * max(1, max visible z) off the flagged pixels -- the project's 1e-5 colour bar for a channel
    in [0, 1], scaled to the channel's range;
  * median depth: equal to the reference bit for bit off the flagged pixels (a copied depth; depths are bit-exact);
  * alpha: equal to 1 - final_T (the exported one) bit for bit, everywhere;
  * flagged = the oracle's threshold-ambiguous pixels (oracle.with_rects, want_ambig=True) plus the median-ambiguous ones
    (aux_ref: some T after a blended entry within 1e-4 relative of 0.5); each share at most 0.1 %.
"""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import camera_cases as cc

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
FLAG_MAX_FRACTION = 1e-3
MAPS = ("depth", "alpha", "median_depth")
BG = np.array([0.1, 0.3, 0.2], np.float32)


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


def maps_of(C_, P, H, W, fout, maps=MAPS, checks=True):
    R, _, _, geom, binning, img = fout
    return C_.aux_maps(P, R, H, W, geom, binning, img, maps=maps, checks=checks)


def same_maps(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)


def consistent(C_, P, H, W, fout, got):
    """T_check == final_T and n_check == n_contrib, bit for bit, on every pixel; alpha == 1 - final_T."""
    ex = C_.export_binning(P, fout[0], H, W, fout[3], fout[4], fout[5])
    assert torch.equal(got["T_check"].reshape(-1), ex["final_T"]), "the pass's own final T is not the forward's"
    assert torch.equal(got["n_check"].reshape(-1), ex["n_contrib"]), "the pass's own last contributor is not the forward's"
    if "alpha" in got:
        assert torch.equal(got["alpha"].reshape(-1), 1.0 - ex["final_T"])
    return ex


def parity(C_, cam, g, H, W, tag, min_median=0.2):
    """The exact-size forward, the maps, and every bar of the module's docstring -> (forward's result, maps, flagged shares)."""
    P = len(g["means3D"])
    fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
    got = maps_of(C_, P, H, W, fout)
    for k in MAPS:
        assert got[k].shape == (1, H, W) and got[k].dtype == torch.float32
    consistent(C_, P, H, W, fout, got)
    ref = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                      cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                      want_ambig=True)
    if C_.tight_rects():
        rects = C_.export_rects(P, fout[3]).cpu().numpy()
        rects[ref["radii"] <= 0] = 0
        ref = orc.with_rects(ref, rects, want_ambig=True)
    st = ref["state"]
    want = ar.aux_ref(st)
    amb, med = ref["ambig"] != 0, want["median_ambig"]
    print(f"[aux maps {tag}] oracle-ambiguous {100 * amb.mean():.4f} %, median-ambiguous {100 * med.mean():.4f} % "
          f"(cap {100 * FLAG_MAX_FRACTION:.2f} % each)")
    assert amb.mean() <= FLAG_MAX_FRACTION and med.mean() <= FLAG_MAX_FRACTION
    ok = ~(amb | med)
    zmax = float(st["depths"][st["radii"] > 0].max())
    depth = got["depth"][0].cpu().numpy()
    err = np.abs(depth - want["depth"])[ok].max()
    print(f"[aux maps {tag}] depth error {err:.3e} (bar {1e-5 * max(1.0, zmax):.3e}, max visible z {zmax:.2f})")
    assert err <= 1e-5 * max(1.0, zmax)
    median = got["median_depth"][0].cpu().numpy()
    np.testing.assert_array_equal(median.view(np.uint32)[ok], want["median_depth"].view(np.uint32)[ok])
    assert (want["median_depth"] > 0).mean() > min_median, "the case must bring pixels below T = 0.5"
    empty = (st["n_contrib"].reshape(H, W) == 0) & ~amb
    for k in MAPS:
        assert not got[k][0].cpu().numpy()[empty].any(), k
    return fout, got


def test_parity_with_the_reference():
    """Scene A (P = 2000, 100x70: partial tiles on both axes, mixed degrees).  Measured on the CPU over the reference's lists
    (oracle.forward, its default ambig_rel): 0.0429 % oracle-ambiguous, 0.0571 % median-ambiguous.  Measured on an MI355X over
    the lists the forward binned (printed by the test): the same 0.0429 % and 0.0571 %; depth error 2.4e-6 against a bar of
    1.27e-4 (max visible z 12.74)."""
    from diff_gaussian_rasterization import _C
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    parity(_C, cam, g, kw["H"], kw["W"], "scene A")


@pytest.mark.parametrize("name", ["A", "B"])
def test_self_consistency(C_, name):
    """The pass's own final T and last contributor are the forward's, bit for bit, on every pixel -- on scene A and on
    scene B, whose heaviest tile list is long enough for the forward to leave segment checkpoints (2 * 128 entries)."""
    kw = ar.SCENE_A if name == "A" else ar.SCENE_B
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    C_.hint_next_forward(True)   # as a training step: checkpoints are only left for a backward
    fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
    got = maps_of(C_, P, H, W, fout)
    ex = consistent(C_, P, H, W, fout, got)
    lens = (ex["ranges"][:, 1] - ex["ranges"][:, 0]).cpu().numpy()
    print(f"[aux maps scene {name}] heaviest tile list {lens.max()} entries, deepest contributor {int(ex['n_contrib'].max())}")
    if name == "B":
        assert lens.max() >= 2 * 128, "scene B must have a list the forward segments"
        assert int(ex["n_contrib"].max()) > 64, "and a walk of more than one chunk"


def test_every_forward_path_leaves_the_same_maps(C_, golden_dir):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    scaling, rotation = dev(np.log(g["scales"]).astype(np.float32)), dev(g["rotations"])
    scales, rotations = C_.activate_params(scaling, rotation)
    args = forward_args(g, cam, H, W, scales, rotations)
    exact = C_._forward_common(None, *args, exact=True)
    want = maps_of(C_, P, H, W, exact)
    consistent(C_, P, H, W, exact, want)
    assert float(want["depth"].max()) > 1.0 and float(want["median_depth"].max()) > 1.0
    # the reserved (graph) path, twice: the second pass of a shape is the replayed one
    reserve = int(exact[0].pairs * 1.25) + 4096
    for _ in range(2):
        reserved = C_._forward_common(None, *args, exact=False, _reserve=reserve)
        assert reserved[0].ticket > 0, "the reserved path was not taken"
        same_maps(maps_of(C_, P, H, W, reserved), want, "reserved")
    # a lean geometry blob (a forward no backward will follow)
    C_.hint_next_forward(False)
    lean = C_._forward_common(None, *args, exact=True)
    C_.hint_next_forward(True)
    full = C_._forward_common(None, *args, exact=True)
    assert lean[3].numel() < full[3].numel(), "the hint did not select the lean blob"
    same_maps(maps_of(C_, P, H, W, lean), want, "lean")
    same_maps(maps_of(C_, P, H, W, full), want, "full")
    # from the raw parameters
    sh = dev(g["sh"])
    params = C_.rasterize_gaussian_params(args[0], args[1], sh[:, :1].contiguous(), sh[:, 1:].contiguous(), args[15], args[3],
                                          scaling, rotation, 1.0, args[8], args[9], cam.tanfovx, cam.tanfovy, H, W, args[16],
                                          False, False, exact=True)
    assert torch.equal(params[1], exact[1])
    same_maps(maps_of(C_, P, H, W, params), want, "raw parameters")
    # the ctypes binding against the compiled one
    was = C_.set_binding("ctypes")
    try:
        assert C_.binding() == "ctypes"
        plain = maps_of(C_, P, H, W, exact)
    finally:
        C_.set_binding(was)
    assert C_.binding() == "torch"
    same_maps(plain, want, "ctypes binding")


def test_ragged_and_quantised_forwards_leave_the_same_maps(C_, golden_dir):
    """The quantised forward of the tests/golden P200 model against the ragged inference forward of its decoded model
    (asserted bit-identical by tests/test_quantised_gpu.py), exact and reserved."""
    from r3dgs_quantised import QuantisedModel
    from tests import test_quantised_gpu as tq
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    inputs = tq.ragged_inputs(C_, qm)
    c = tq.camera("131x77", T=(0.1, -0.05, 4.0))
    ragged = tq.ragged_forward(C_, qm, inputs, c)
    want = maps_of(C_, qm.P, c.H, c.W, ragged)
    consistent(C_, qm.P, c.H, c.W, ragged, want)
    assert float(want["alpha"].max()) > 0.5 and float(want["depth"].max()) > 1.0
    quant = tq.quantised_forward(C_, qm, c)
    got = maps_of(C_, qm.P, c.H, c.W, quant)
    consistent(C_, qm.P, c.H, c.W, quant, got)
    same_maps(got, want, "quantised")
    reserve = int(ragged[0].pairs * 1.25) + 4096
    same_maps(maps_of(C_, qm.P, c.H, c.W, tq.ragged_forward(C_, qm, inputs, c, exact=False, reserve=reserve)), want, "ragged, reserved")
    same_maps(maps_of(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c, exact=False, reserve=reserve)), want, "quantised, reserved")


def test_the_blobs_are_left_as_the_backward_needs_them(C_):
    """forward -> aux -> backward against forward -> backward: every gradient tensor bit-identical."""
    import synth_scene as ss
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    args = forward_args(g, cam, H, W)
    dl = dev(ss.upstream_grad(W, H, seed=3) * (W * H))
    (bg, m3, colors, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args

    def grads(with_aux, exact):
        C_.hint_next_forward(True)
        fout = (C_._forward_common(None, *args, exact=True) if exact else C_.rasterize_gaussians(*args))
        if with_aux:
            maps_of(C_, P, H, W, fout)
        R, _, radii, geom, binning, img = fout
        return C_.rasterize_gaussians_backward(bg, m3, radii, colors, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom,
                                               R, binning, img, 0.0, False)
    for exact in (True, False):
        plain, after = grads(False, exact), grads(True, exact)
        assert len(plain) == len(after) == 8
        for k, (a, b) in enumerate(zip(plain, after)):
            assert torch.equal(a, b), (exact, k)
        assert float(plain[3].abs().max()) > 0


def test_empty_model_and_all_culled(C_):
    H, W = 40, 56
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=64, W=W, H=H))
    empty = {k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()}
    fout = C_._forward_common(None, *forward_args(empty, cam, H, W), exact=True)
    assert fout[3].numel() == 0
    got = maps_of(C_, 0, H, W, fout)
    for k in MAPS + ("T_check", "n_check"):
        assert got[k].numel() == H * W and not got[k].any(), k
    assert got["depth"].shape == (1, H, W) and got["depth"].is_cuda
    behind = dict(g)
    behind["means3D"] = g["means3D"].copy()
    behind["means3D"][:, 2] = -np.abs(g["means3D"][:, 2]) - 1.0   # behind the (nearly identity) camera: all culled
    fout = C_._forward_common(None, *forward_args(behind, cam, H, W), exact=True)
    assert int(fout[0]) == 0 and not fout[2].any()
    got = maps_of(C_, 64, H, W, fout)
    consistent(C_, 64, H, W, fout, got)
    for k in MAPS + ("n_check",):
        assert not got[k].any(), k
    assert (got["T_check"] == 1.0).all()


def test_17x17_image():
    """One pixel past a tile on both axes.  Measured on the CPU: no flagged pixel (289 pixels: the cap allows none)."""
    from diff_gaussian_rasterization import _C
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    parity(_C, cam, g, kw["H"], kw["W"], "17x17")


@pytest.mark.parametrize("name", sorted(ar.SMALL))
def test_small_models_on_a_17x19_image(name):
    """P = 65 (one Gaussian past a wave) and P = 1 on 17x19, partial tiles on both axes: every bar of `parity`, except that only
    some pixel, not a fifth of them, has to have a median depth (tests/aux_ref.py: 10.5 % and one pixel)."""
    from diff_gaussian_rasterization import _C
    kw = ar.SMALL[name]
    cam, g, _ = ar.make_scene(kw)
    parity(_C, cam, g, kw["H"], kw["W"], name, min_median=0.0)


def test_portrait_camera_with_non_square_pixels():
    """tests/camera_cases.py 'portrait_far' (117x203, fx != fy, far-rotated).  Measured on the CPU over the reference's lists:
    0.0168 % oracle-ambiguous, 0.0421 % median-ambiguous; the same on an MI355X, depth error 1.5e-5 against a bar of 1.2e-4."""
    from diff_gaussian_rasterization import _C
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", ar.PORTRAIT["P"], ar.PORTRAIT["seed"])
    assert cam.image_height > cam.image_width and abs(cc.CAMERAS[ar.PORTRAIT["camera"]]["gpu"][2] / cc.CAMERAS[ar.PORTRAIT["camera"]]["gpu"][3] - 1) >= 0.2
    parity(_C, cam, g, cam.image_height, cam.image_width, "portrait_far")


def test_each_output_alone(C_):
    """Every single-output call (the other pointers NULL) writes what the full call writes, under both bindings."""
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
    want = maps_of(C_, P, H, W, fout)
    for binding in ("torch", "ctypes"):
        was = C_.set_binding(binding)
        try:
            for k in MAPS:
                one = maps_of(C_, P, H, W, fout, maps=(k,), checks=False)
                assert set(one) == {k} and torch.equal(one[k], want[k]), (binding, k)
            only_checks = maps_of(C_, P, H, W, fout, maps=(), checks=True)
            assert set(only_checks) == {"T_check", "n_check"}
            assert torch.equal(only_checks["T_check"], want["T_check"]) and torch.equal(only_checks["n_check"], want["n_check"])
        finally:
            C_.set_binding(was)
    # straight at the C ABI: n_check alone, then nothing at all
    import ctypes
    n = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    R, _, _, geom, binning, img = fout
    st = C_._lib.r3dgs_aux_maps(P, R.capacity, W, H, geom.data_ptr(), binning.data_ptr(), img.data_ptr(), None, None, None, None,
                                n.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0 and torch.equal(n, want["n_check"])
    assert C_._lib.r3dgs_aux_maps(P, R.capacity, W, H, geom.data_ptr(), binning.data_ptr(), img.data_ptr(), None, None, None, None,
                                  None, None) == 0


def test_captured_launch_replays_over_fixed_buffers(C_):
    """Only the aux launch is captured, over fixed state buffers and fixed outputs; replayed after two different forwards
    whose blobs were copied into those buffers, each replay equals the direct call on the forward's own blobs."""
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
    assert all(a.numel() == b.numel() for a, b in zip(first[3:], second[3:]))
    fixed = [torch.empty_like(t) for t in first[3:]]
    for dst, src in zip(fixed, first[3:]):
        dst.copy_(src)
    call = lambda blobs: C_.aux_maps(P, first[0], H, W, *blobs, maps=MAPS, checks=True)   # noqa: E731
    call(fixed)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = call(fixed)
    for fout in (first, second, first):
        for dst, src in zip(fixed, fout[3:]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        same_maps({k: v.clone() for k, v in static.items()}, call(list(fout[3:])), "replay")
    assert not torch.equal(call(list(first[3:]))["depth"], call(list(second[3:]))["depth"])


def test_render_with_aux(C_, monkeypatch):
    import r3dgs_render
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussian_params
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    sh = dev(g["sh"])
    pc = NS(_xyz=dev(g["means3D"]).requires_grad_(True), _features_dc=sh[:, :1].contiguous().requires_grad_(True),
            _features_rest=sh[:, 1:].contiguous().requires_grad_(True), _opacity=dev(g["opacity"]).requires_grad_(True),
            _scaling=dev(np.log(g["scales"]).astype(np.float32)).requires_grad_(True), _rotation=dev(g["rotations"]).requires_grad_(True),
            _degrees=dev(g["degrees"]), active_sh_degree=3, max_sh_degree=3)
    view = NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = dev(BG)
    leaves = (pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation)

    def grads_of(out):
        for t in leaves:
            t.grad = None
        (out["render"] * dev(np.linspace(0.5, 1.5, 3 * H * W, dtype=np.float32).reshape(3, H, W))).sum().backward()
        return [t.grad.clone() for t in leaves]

    # without aux: the existing path's dictionary and image, and no aux launch
    real = C_.aux_maps
    monkeypatch.setattr(C_, "aux_maps", None)
    monkeypatch.setattr(r3dgs_render, "aux_maps", None)
    plain = r3dgs_render.render(view, pc, pipe, bg)
    assert set(plain) == {"render", "viewspace_points", "visibility_filter", "radii", "FPS"}
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, bg, 1.0, view.world_view_transform, view.full_proj_transform, 3,
                                       view.camera_center, False, False)
    image, radii = rasterize_gaussian_params(pc._xyz, torch.zeros_like(pc._xyz), pc._features_dc, pc._features_rest, pc._degrees,
                                             pc._opacity, pc._scaling, pc._rotation, rs, 0.0)
    assert torch.equal(plain["render"], image) and torch.equal(plain["radii"], radii)
    plain_grads = grads_of(plain)
    monkeypatch.undo()
    assert C_.aux_maps is real

    out = r3dgs_render.render(view, pc, pipe, bg, aux=MAPS)
    assert set(out) == set(plain) | set(MAPS)
    assert torch.equal(out["render"], plain["render"]) and torch.equal(out["radii"], plain["radii"])
    for k in MAPS:
        assert out[k].shape == (1, H, W) and out[k].dtype == torch.float32 and out[k].is_cuda
        assert not out[k].requires_grad and out[k].grad_fn is None, k
    direct = C_.rasterize_gaussian_params(bg, *[t.detach() for t in (pc._xyz, pc._features_dc, pc._features_rest)], pc._degrees,
                                          pc._opacity.detach(), pc._scaling.detach(), pc._rotation.detach(), 1.0,
                                          view.world_view_transform, view.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W,
                                          view.camera_center, False, False, exact=True)
    want = maps_of(C_, P, H, W, direct, checks=False)
    same_maps({k: out[k] for k in MAPS}, want, "render(aux=...)")
    assert float(out["alpha"].max()) > 0.9 and float(out["median_depth"].max()) > 1.0
    for a, b in zip(grads_of(out), plain_grads):   # the maps in between change nothing for the backward
        assert torch.equal(a, b)
    subset = r3dgs_render.render(view, pc, pipe, bg, aux=("alpha",))
    assert set(subset) == set(plain) | {"alpha"} and torch.equal(subset["alpha"], want["alpha"])
    with torch.no_grad():   # a rendering: the lean blob
        same_maps({k: v for k, v in r3dgs_render.render(view, pc, pipe, bg, aux=MAPS).items() if k in MAPS}, want, "no_grad")

    # a quantised model
    from tests import test_quantised_gpu as tq
    qm, _ = tq.model("37-0-150-70")
    c = tq.camera("131x77")
    qview = NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm, full_proj_transform=c.pm,
               camera_center=c.cp)
    qout = r3dgs_render.render(qview, qm, pipe, c.bg, aux=MAPS)
    qwant = maps_of(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c), checks=False)
    same_maps({k: qout[k] for k in MAPS}, qwant, "render(QuantisedModel, aux=...)")
    assert set(qout) == set(plain) | set(MAPS) and float(qout["alpha"].max()) > 0.5
