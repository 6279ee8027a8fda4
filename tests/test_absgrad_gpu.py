"""GPU checks of the absolute screen-space gradients: render(..., absgrad=True) against the float64 restatement
tests/absgrad_ref.py on the smallest scenes that reach every path (partial tiles, a list of several chunks with and without
segments, a portrait camera with fx != fy), the exact zeros, abs >= |signed|, and the bit identities -- the signed gradients
with the option on, run to run, plain / abs passes alternating (the graph keying), reserved == exact, compiled == ctypes
binding, raw-parameter == activated path, a dirty workspace, a captured graph -- and the statistics call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth_scene as ss
from oracle import oracle as orc
from tests import absgrad_ref as ag
from tests import camera_cases as cc

pytestmark = pytest.mark.gpu
REL = 1e-4                  # the project's gradient bar, relative to max|ref| per column
AMBIG_MAX_FRACTION = 1e-3


def dv(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


class Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


PipeExact = type("PipeExact", (), dict(debug=True, compute_cov3D_python=False, convert_SHs_python=False))


class Cam:
    def __init__(self, cam, W, H):
        self.FoVx, self.FoVy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
        self.image_height, self.image_width = H, W
        self.world_view_transform, self.full_proj_transform = dv(cam.world_view_transform), dv(cam.full_proj_transform)
        self.camera_center = dv(cam.camera_center)


class Model:
    """GaussianModel-shaped stand-in over a synth_scene cloud: raw leaves, the reference's activations."""
    max_sh_degree = active_sh_degree = 3
    leaves = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")

    def __init__(self, g):
        self._xyz = dv(g["means3D"]).requires_grad_()
        sh = dv(g["sh"])
        self._features_dc = sh[:, :1].contiguous().requires_grad_()
        self._features_rest = sh[:, 1:].contiguous().requires_grad_()
        self._opacity = dv(g["opacity"]).requires_grad_()
        self._scaling = torch.log(dv(g["scales"])).requires_grad_()
        self._rotation = dv(g["rotations"]).requires_grad_()
        self._degrees = dv(g["degrees"])

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: F.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))


class Scene:
    def __init__(self, name, cam, g, bg, W, H, seed):
        self.name, self.g, self.W, self.H = name, g, W, H
        self.cam, self.bg = Cam(cam, W, H), dv(bg)
        ref = orc.forward(bg, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                          cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                          want_ambig=True, ambig_rel=1e-5)
        assert ref["ambig"].mean() <= AMBIG_MAX_FRACTION
        dl = ag.masked_upstream(ss.upstream_grad(W, H, seed=seed) * (W * H), ref["ambig"])   # masked on both sides
        self.ref, self.radii = ag.absgrad_ref(ref["state"], dl, ref["ambig"]), ref["radii"]
        self.dl = dv(dl)

    def run(self, absgrad=True, pipe=Pipe, **kw):
        """-> dict(image, radii, grad (viewspace_points.grad), abs (or None), leaves)"""
        import r3dgs_render
        pc = Model(self.g)
        out = r3dgs_render.render(self.cam, pc, pipe, self.bg, absgrad=absgrad, **kw)
        (out["render"] * self.dl).sum().backward()
        vp = out["viewspace_points"]
        return dict(image=out["render"].detach().clone(), radii=out["radii"].clone(), grad=vp.grad.clone(),
                    abs=getattr(vp, "absgrad", None), leaves=[getattr(pc, k).grad.clone() for k in Model.leaves], vp=vp)


@pytest.fixture(scope="module")
def scenes():
    """The reference of every scene, computed once and left unchanged."""
    out = {}
    for k, (name, kw) in enumerate((("tiles", ag.SCENE_TILES), ("one_tile", ag.SCENE_ONE_TILE))):
        cam, g, bg = ag.make_scene(kw)
        out[name] = Scene(name, cam, g, bg, kw["W"], kw["H"], 40 + k)
    cam, g = cc.cloud(ag.PORTRAIT["camera"], "gpu", ag.PORTRAIT["P"], ag.PORTRAIT["seed"])
    out["portrait"] = Scene("portrait", cam, g, np.array([0.1, 0.3, 0.2], np.float32), cam.image_width, cam.image_height, 42)
    return out


def gpu_binning(sc):
    """What the library itself binned for scene `sc` (exact-size forward): dict(tiles_touched [P], ranges [tiles,2], ...)."""
    from diff_gaussian_rasterization import _C
    g = sc.g
    none = torch.Tensor([])
    fwd = _C.rasterize_gaussians(sc.bg, dv(g["means3D"]), none, dv(g["opacity"]), dv(g["scales"]), dv(g["rotations"]), 1.0, none,
                                 sc.cam.world_view_transform, sc.cam.full_proj_transform, math.tan(sc.cam.FoVx * 0.5),
                                 math.tan(sc.cam.FoVy * 0.5), sc.H, sc.W, dv(g["sh"]), dv(g["degrees"]), sc.cam.camera_center,
                                 False, True)
    return _C.export_binning(g["means3D"].shape[0], int(fwd[0]), sc.H, sc.W, fwd[3], fwd[4], fwd[5])


def same_signed(a, b):
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["radii"], b["radii"]) and torch.equal(a["grad"], b["grad"])
    for x, y in zip(a["leaves"], b["leaves"]):
        assert torch.equal(x, y)


def held(sc, r, what):
    """The abs columns of run `r` against the restatement, and the properties every result has."""
    a = r["abs"]
    assert a is not None and a.dtype == torch.float32 and tuple(a.shape) == (sc.g["means3D"].shape[0], 3) and not a.requires_grad
    got = a.cpu().numpy().astype(np.float64)
    for col in range(2):
        scale = np.abs(sc.ref["abs"][:, col]).max()
        err = np.abs(got[:, col] - sc.ref["abs"][:, col]).max()
        print(f"{sc.name} {what} abs[{col}]: err / max|ref| = {err / scale:.2e}")
        assert err <= REL * scale, (sc.name, what, col, err / scale)
    assert not got[:, 2].any(), "third column"
    assert not got[sc.radii <= 0].any(), "rows of culled Gaussians"
    assert not got[~(sc.ref["abs"] > 0).any(axis=1)].any(), "rows of Gaussians that reach no pixel"
    signed = r["grad"].cpu().numpy().astype(np.float64)
    assert (got[:, :2] >= np.abs(signed[:, :2]) - 1e-6 * got.max()).all()


@pytest.mark.parametrize("name", ["tiles", "one_tile", "portrait"])
def test_abs_columns_against_the_restatement(scenes, name):
    sc = scenes[name]
    plain = sc.run(absgrad=False)
    assert plain["abs"] is None
    r = sc.run()
    held(sc, r, "default")
    same_signed(r, plain)          # the nine signed gradients, the image and the radii: bit-identical with the option on
    again = sc.run()
    assert torch.equal(again["abs"], r["abs"]), "run to run"
    exact = sc.run(pipe=PipeExact)   # exact-size path == reserved path
    assert torch.equal(exact["abs"], r["abs"])


def test_plain_and_abs_passes_alternate(scenes):
    """One process, both graphs of one shape: each pass gets its own."""
    sc = scenes["tiles"]
    first_abs, first_plain = sc.run(), sc.run(absgrad=False)
    for _ in range(2):
        p, a = sc.run(absgrad=False), sc.run()
        same_signed(p, first_plain)
        same_signed(a, first_abs)
        assert p["abs"] is None and torch.equal(a["abs"], first_abs["abs"])


@pytest.mark.parametrize("segments", [1, 0])
def test_a_list_of_several_chunks_with_and_without_segments(scenes, segments):
    """One tile, one list of more than two 64-entry chunks, with the segment switch on and off.  (A one-tile pass has no room for
    a second unit, so this list is never split: the split walk is test_segmented_walk_of_a_long_list.)"""
    from diff_gaussian_rasterization import _C
    sc = scenes["one_tile"]
    before = _C.set_bwd_segments(segments)
    try:
        r = sc.run()
    finally:
        _C.set_bwd_segments(before)
    held(sc, r, f"segments={segments}")


@pytest.mark.parametrize("order", [1, 0])
def test_with_and_without_the_unit_order(scenes, order):
    from diff_gaussian_rasterization import _C
    sc = scenes["tiles"]
    want = sc.run()
    before = _C.set_tile_order(order)
    try:
        r = sc.run()
    finally:
        _C.set_tile_order(before)
    held(sc, r, f"unit order={order}")
    assert torch.equal(r["abs"], want["abs"])   # every unit's arithmetic is its own


def test_segmented_walk_of_a_long_list():
    """3 x 2 tiles under enough faint Gaussians that a list is long (>= 2 x 128 entries), its pixels look deep into it (opacity
    0.04: a pixel is not saturated before entry 128) and the pass has room for extra units (>= 1024 pairs: a list of the unit
    order takes its tiles plus pairs / 128 / 8 segments -- a one-tile image never has room), so the walk is split: segmented ==
    unsegmented to the bar (T is recovered from a checkpoint), not bitwise, and both against the restatement."""
    from diff_gaussian_rasterization import _C
    kw = dict(ag.SCENE_TILES, P=1800, gseed=33, scale_mu=0.2)
    cam, g, bg = ag.make_scene(kw)
    g = dict(g, opacity=np.full_like(g["opacity"], -3.2))   # raw: sigmoid(-3.2) = 0.039
    sc = Scene("long_list", cam, g, bg, kw["W"], kw["H"], 45)
    binned = gpu_binning(sc)
    lengths = (binned["ranges"][:, 1] - binned["ranges"][:, 0])
    assert int(lengths.max()) >= 2 * 128, "the longest list the library binned is too short to be split"
    assert int(lengths.sum()) >= 1024, "the pass has no room for a second unit of a tile"
    assert int(binned["n_contrib"].max()) > 128, "no pixel looks past the first segment"
    on = sc.run()
    before = _C.set_bwd_segments(0)
    try:
        off = sc.run()
    finally:
        _C.set_bwd_segments(before)
    held(sc, on, "segmented")
    held(sc, off, "unsegmented")
    scale = off["abs"].abs().amax(dim=0)[:2]
    assert ((on["abs"] - off["abs"]).abs().amax(dim=0)[:2] <= REL * scale).all()
    # the split walk starts pixels from the forward's checkpoints instead of its own division chain: other roundings
    assert not (torch.equal(on["abs"], off["abs"]) and torch.equal(on["grad"], off["grad"])), "the list was not walked in segments"


def test_runs_that_span_several_pair_groups():
    """A few very large Gaussians over 13 x 12 tiles: a Gaussian's pairs cover whole 64-pair groups of the slab, so its abs sums
    are put together by the finish kernel from a trailing piece and several leading ones."""
    kw = dict(P=24, W=208, H=192, f=150.0, cam_seed=4, gseed=34, degree_mode="mixed", scale_mu=1.2)
    cam, g, bg = ag.make_scene(kw)
    sc = Scene("wide_splats", cam, g, bg, kw["W"], kw["H"], 46)
    assert int(gpu_binning(sc)["tiles_touched"].max()) >= 129, "no run covers a whole 64-pair group between two others"
    r = sc.run()
    held(sc, r, "default")
    assert torch.equal(sc.run()["abs"], r["abs"])


def test_the_instantiations_that_repeat_the_pre_test():
    """blend_bwd_kernel<4, false, *, true>: taken when the forward's quad masks are not kept, which the library reads from the
    environment once per process -- so a child process runs the restatement and the unit-order tests with it off."""
    import os
    import subprocess
    import sys
    if os.environ.get("R3DGS_KEEP_QUAD_MASKS") == "0":
        pytest.skip("this is the child process")
    env = dict(os.environ, R3DGS_KEEP_QUAD_MASKS="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-p", "no:cacheprovider", "-k",
                          "test_abs_columns_against_the_restatement or test_with_and_without_the_unit_order"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "5 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_bindings_and_paths_agree_bit_for_bit(scenes):
    from diff_gaussian_rasterization import _C
    sc = scenes["tiles"]
    want = sc.run()
    before = _C.set_binding("ctypes")
    try:
        r = sc.run()
    finally:
        _C.set_binding(before)
    assert torch.equal(r["abs"], want["abs"])
    same_signed(r, want)
    # the activated path (the raw-parameter route refused by a pipe flag it does not cover ... here: precomputed nothing, but
    # scales / rotations activated in torch): the same 2D records, so the same abs columns
    import diff_gaussian_rasterization as dgr
    pc = Model(sc.g)
    rs = dgr.GaussianRasterizationSettings(sc.H, sc.W, math.tan(sc.cam.FoVx * 0.5), math.tan(sc.cam.FoVy * 0.5), sc.bg, 1.0,
                                           sc.cam.world_view_transform, sc.cam.full_proj_transform, 3, sc.cam.camera_center,
                                           False, False)
    means2D = torch.zeros_like(pc._xyz, requires_grad=True) + 0
    means2D.retain_grad()
    scales, rots = _C.activate_params(pc._scaling.detach(), pc._rotation.detach())
    with dgr.absgrad():
        image, radii = dgr.GaussianRasterizer(rs)(means3D=pc._xyz, means2D=means2D, shs=pc.get_features, degrees=pc._degrees,
                                                  opacities=pc._opacity, scales=scales, rotations=rots)
    (image * sc.dl).sum().backward()
    assert torch.equal(means2D.absgrad, want["abs"]) and torch.equal(means2D.grad, want["grad"])


def test_a_dirty_workspace_gives_the_same_answer(scenes):
    """The C entry point with a workspace of 0xFF bytes and one of zeros: the same output."""
    from diff_gaussian_rasterization import _C
    sc = scenes["one_tile"]
    g = sc.g
    P = g["means3D"].shape[0]
    m3, op, sh, deg = dv(g["means3D"]), dv(g["opacity"]), dv(g["sh"]), dv(g["degrees"])
    sca, rot = dv(g["scales"]), dv(g["rotations"])
    tx, ty = math.tan(sc.cam.FoVx * 0.5), math.tan(sc.cam.FoVy * 0.5)
    none = torch.Tensor([])
    fwd = _C.rasterize_gaussians(sc.bg, m3, none, op, sca, rot, 1.0, none, sc.cam.world_view_transform,
                                 sc.cam.full_proj_transform, tx, ty, sc.H, sc.W, sh, deg, sc.cam.camera_center, False, True)
    R, radii, geom, binning, img = int(fwd[0]), fwd[2], fwd[3], fwd[4], fwd[5]
    n = _C._lib.r3dgs_absgrad_workspace_floats(R)
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((n * 4,), fill, dtype=torch.uint8, device="cuda")
        o = {k: torch.empty(s, device="cuda") for k, s in dict(m2=(P, 3), op=(P, 1), col=(P, 3), m3=(P, 3), cov=(P, 6),
                                                                 sh=(P, 16, 3), sc=(P, 3), rot=(P, 4), abs=(P, 3)).items()}
        p = lambda t: C.c_void_p(t.data_ptr())
        st = _C._lib.r3dgs_backward_absgrad(
            P, p(deg), 16, R, p(sc.bg), sc.W, sc.H, p(m3), p(sh), None, p(sca), 1.0, p(rot), None, p(sc.cam.world_view_transform),
            p(sc.cam.full_proj_transform), p(sc.cam.camera_center), tx, ty, p(radii), p(geom), p(binning), p(img), p(sc.dl),
            p(o["m2"]), None, p(o["op"]), p(o["col"]), p(o["m3"]), p(o["cov"]), p(o["sh"]), p(o["sc"]), p(o["rot"]), 0.0, 0,
            C.c_void_p(torch.cuda.current_stream().cuda_stream), p(o["abs"]), p(ws), n)
        assert st == 0, _C._lib.r3dgs_last_error().decode()
        torch.cuda.synchronize()
        outs.append(o["abs"].clone())
    assert torch.equal(outs[0], outs[1])
    err = (outs[0].cpu().numpy()[:, :2] - sc.ref["abs"]).__abs__().max(axis=0)
    assert (err <= REL * np.abs(sc.ref["abs"]).max(axis=0)).all()


@pytest.mark.parametrize("absgrad", [True, False])
def test_a_captured_graph_replays_to_the_eager_result(scenes, absgrad):
    """Forward + loss + backward inside torch.cuda.graph, with the option on and off.  Captured on the stream the warm-up ran on
    (the library keeps its argument blocks per stream and shape: nothing is allocated under capture) and with the strict mode
    off (a strict forward waits on the host for its pass header, which a capture never publishes)."""
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    sc = scenes["tiles"]
    want = sc.run(absgrad=absgrad)
    pc = Model(sc.g)
    side = torch.cuda.Stream()
    before = _C.is_strict()
    _C.set_strict(False)
    try:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up outside the capture: the library's graphs of this stream and shape exist
            for _ in range(2):
                out = r3dgs_render.render(sc.cam, pc, Pipe, sc.bg, absgrad=absgrad)
                (out["render"] * sc.dl).sum().backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for k in Model.leaves:
            getattr(pc, k).grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = r3dgs_render.render(sc.cam, pc, Pipe, sc.bg, absgrad=absgrad)
            (out["render"] * sc.dl).sum().backward()
    finally:
        _C.set_strict(before)
    vp = out["viewspace_points"]
    vp.grad.zero_()
    out["render"].detach().zero_()
    if absgrad:
        vp.absgrad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(vp.grad, want["grad"]) and torch.equal(out["render"].detach(), want["image"])
    for k, w in zip(Model.leaves, want["leaves"]):
        assert torch.equal(getattr(pc, k).grad, w), k
    if absgrad:
        assert torch.equal(vp.absgrad, want["abs"])
    else:
        assert not hasattr(vp, "absgrad")


def test_a_capture_of_a_shape_the_stream_has_not_run_is_refused(scenes):
    """Nothing may be allocated inside the caller's capture: the pass says what to do instead of failing in the runtime."""
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    sc = scenes["tiles"]
    sc.run()                      # the view is known (a reservation exists), but not on the stream captured below
    pc = Model(sc.g)
    fresh = torch.cuda.Stream()
    before = _C.is_strict()
    _C.set_strict(False)
    try:
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="has not run on this stream"):
            with torch.cuda.graph(graph, stream=fresh):
                r3dgs_render.render(sc.cam, pc, Pipe, sc.bg, absgrad=True)
    finally:
        _C.set_strict(before)
    torch.cuda.synchronize()
    sc.run()                      # and the library goes on as before


def test_no_grad_and_a_frozen_model_are_no_ops(scenes):
    import r3dgs_render
    sc = scenes["tiles"]
    pc = Model(sc.g)
    with torch.no_grad():
        out = r3dgs_render.render(sc.cam, pc, Pipe, sc.bg, absgrad=True)
    assert not hasattr(out["viewspace_points"], "absgrad")
    frozen = Model(sc.g)
    for k in Model.leaves:
        getattr(frozen, k).requires_grad_(False)
    out = r3dgs_render.render(sc.cam, frozen, Pipe, sc.bg, absgrad=True)
    assert not out["render"].requires_grad or not hasattr(out["viewspace_points"], "absgrad")
    import diff_gaussian_rasterization as dgr
    assert dgr._absgrad_request.on is False and dgr._absgrad_request.scope is False


def test_densification_statistics_take_the_abs_signal(scenes):
    import r3dgs_train_stats as ts
    sc = scenes["tiles"]
    r = sc.run()
    P = r["abs"].shape[0]
    pc = type("Stats", (), {})()
    pc.xyz_gradient_accum, pc.denom = torch.zeros(P, 1, device="cuda"), torch.zeros(P, 1, device="cuda")
    pc.max_radii2D = torch.zeros(P, device="cuda")
    ts.add_densification_stats_absgrad(pc, r["vp"], r["radii"])
    vis = r["radii"] > 0
    want = torch.zeros(P, 1, device="cuda")
    want[vis] += torch.norm(r["abs"][vis, :2], dim=-1, keepdim=True)
    assert torch.equal(pc.xyz_gradient_accum, want) and torch.equal(pc.denom, vis.float().unsqueeze(1))
    assert (pc.xyz_gradient_accum[vis] >= torch.norm(r["grad"][vis, :2], dim=-1, keepdim=True) - 1e-6 * want.max()).all()
