"""GPU tests (-m gpu) of the gradients through the auxiliary maps (include/r3dgs_aux.h r3dgs_aux_maps_backward, csrc/aux_bwd.hip):
against the float64 reference tests/aux_grad_ref.py, against the library's own colour backward fed the colour (z, 1, 0), at the
edge shapes, for determinism and untouched state, inside a captured graph and through r3dgs_render.render(aux_grad=True).

Bar, per tensor (the project's gradient bar): max |got - ref| <= 1e-4 * max |ref|.  The pixels the project flags -- the oracle's
threshold-ambiguous ones and aux_ref's median_ambig ones, at most 0.1 % each -- carry a zero upstream gradient on both sides."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aux_grad_ref as agr
from tests import aux_ref as ar
from tests import camera_cases as cc

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
BG = np.array([0.1, 0.3, 0.2], np.float32)
REL = 1e-4
FLAG_MAX_FRACTION = 1e-3
MAPS = ("depth", "alpha", "median_depth")
NAMES = ("means2D", "means3D", "opacity", "scales", "rotations")


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


def dev(a):
    return EMPTY if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def forward_args(g, cam, H, W, colors=None):
    return (dev(np.zeros(3, np.float32) if colors is not None else BG), dev(g["means3D"]), EMPTY if colors is None else colors,
            dev(g["opacity"]), dev(g["scales"]), dev(g["rotations"]), 1.0, EMPTY, dev(cam.world_view_transform),
            dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, H, W, EMPTY if colors is not None else dev(g["sh"]),
            dev(g["degrees"]), dev(cam.camera_center), False, False)


def upstream(H, W, seed, ok=None):
    """Three seeded upstream gradients [H*W] (float32), zero on the pixels `ok` excludes."""
    rng = np.random.default_rng(seed)
    gs = [rng.uniform(-1.0, 1.0, H * W).astype(np.float32) for _ in range(3)]
    if ok is not None:
        gs = [g * ok.reshape(-1) for g in gs]
    return gs


def call(C_, g, cam, H, W, fout, ups, want=None):
    R, _, radii, geom, binning, img = fout
    return C_.aux_maps_backward(len(g["means3D"]), R, H, W, geom, binning, img, dev(cam.world_view_transform),
                                dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, dev(g["means3D"]), dev(g["scales"]), 1.0,
                                dev(g["rotations"]), EMPTY, radii, *[None if u is None else dev(u) for u in ups],
                                **({} if want is None else {"want": want}))


def held(got, ref, what):
    worst = 0.0
    for k in NAMES:
        a, b = got[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        if k == "means2D":
            assert not a[:, 2].any()
            a = a[:, :2]
        scale = np.abs(b).max()
        err = np.abs(a - b.reshape(a.shape)).max()
        print(f"[aux grad {what}] {k}: max err {err:.3e}, bar {REL * scale:.3e} (max |ref| {scale:.3e})")
        assert err <= REL * scale, (what, k, err, scale)   # (a tensor the reference leaves at zero must be zero: the median
        worst = max(worst, err / scale if scale else 0.0)  # depth alone reaches nothing but means3D)
    assert max(np.abs(np.asarray(ref[k])).max() for k in NAMES) > 0, what
    return worst


class Case:
    """A scene, its exact-size forward on the device, the oracle's state over the device's rects and the unflagged pixels."""

    def __init__(self, C_, cam, g, H, W):
        self.cam, self.g, self.H, self.W, self.P = cam, g, H, W, len(g["means3D"])
        self.fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
        ref = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                          cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                          want_ambig=True)
        if C_.tight_rects():
            rects = C_.export_rects(self.P, self.fout[3]).cpu().numpy()
            rects[ref["radii"] <= 0] = 0
            ref = orc.with_rects(ref, rects, want_ambig=True)
        self.st = ref["state"]
        amb, med = ref["ambig"].reshape(-1) != 0, ar.aux_ref(self.st)["median_ambig"].reshape(-1)
        assert amb.mean() <= FLAG_MAX_FRACTION and med.mean() <= FLAG_MAX_FRACTION
        self.ok = (~(amb | med)).astype(np.float32)
        self._refs = {}

    def ref(self, ups):
        key = tuple(u is not None for u in ups)
        if key not in self._refs:   # computed once per combination of maps, shared, never modified
            g, cam = self.g, self.cam
            self._refs[key] = agr.reference_grads(self.st, g["means3D"], g["opacity"], g["scales"], g["rotations"],
                                                  cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, *ups)
        return self._refs[key]


@pytest.fixture(scope="module")
def scene_a(C_):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    return Case(C_, cam, g, kw["H"], kw["W"])


@pytest.mark.parametrize("which", ["depth", "alpha", "median_depth", "all"])
def test_parity_with_the_float64_reference(C_, scene_a, which):
    """Scene A (P = 2000, 100x70), each map alone and all three, under both settings of set_f64_chain."""
    c = scene_a
    ups = upstream(c.H, c.W, 11, c.ok)
    if which != "all":
        ups = [u if name == which else None for name, u in zip(MAPS, ups)]
    ref = c.ref(ups)
    was = C_.set_f64_chain(True)
    try:
        for f64 in (True, False):
            C_.set_f64_chain(f64)
            held(call(C_, c.g, c.cam, c.H, c.W, c.fout, ups), ref, f"scene A, {which}, f64_chain={f64}")
    finally:
        C_.set_f64_chain(was)


def test_agreement_with_the_colour_backward(C_, scene_a):
    """colors_precomp = (z, 1, 0) over a black background, dL_dout = (g_D, g_A, 0), through the unmodified
    rasterize_gaussians / rasterize_gaussians_backward: the same geometry gradients, and dL_dcolors_precomp[:, 0] is the z
    sum.  The z sum is taken out of the new call's dL_dmeans3D by a second call with every Gaussian's depth gradient routed
    alone: dL_dmeans3D(new) - dL_dmeans3D(colour) = view row 3 (x) dL_dz."""
    c = scene_a
    g, cam, H, W = c.g, c.cam, c.H, c.W
    V = np.asarray(cam.world_view_transform, np.float64).reshape(4, 4)
    z = (np.concatenate([g["means3D"], np.ones((c.P, 1), np.float32)], 1).astype(np.float64) @ V)[:, 2]
    colors = dev(np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32))
    args = forward_args(g, cam, H, W, colors=colors)
    C_.hint_next_forward(True)
    fout = C_._forward_common(None, *args, exact=True)
    gD, gA, _ = upstream(H, W, 12)
    new = call(C_, g, cam, H, W, fout, [gD, gA, None])
    (bg, m3, col, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
    dl = dev(np.stack([gD, gA, np.zeros_like(gD)]).reshape(3, H, W))
    R, _, radii, geom, binning, img = fout
    old = C_.rasterize_gaussians_backward(bg, m3, radii, col, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom, R,
                                          binning, img, 0.0, False)
    m2, dcol, dop, dm3, _, _, dsc, drot = [t.cpu().numpy().astype(np.float64) for t in old]
    dz = dcol[:, 0]
    ref = dict(means2D=m2[:, :2], opacity=dop, scales=dsc, rotations=drot, means3D=dm3 + dz[:, None] * V[:3, 2][None, :])
    held(new, ref, "against the colour backward")
    # the z sum alone: what the new call adds to dL_dmeans3D, projected back on the view's third row
    got_dz = (new["means3D"].cpu().numpy().astype(np.float64) - dm3) @ V[:3, 2] / (V[:3, 2] @ V[:3, 2])
    err, scale = np.abs(got_dz - dz).max(), np.abs(dz).max()
    print(f"[aux grad] z sum against dL_dcolors_precomp[:, 0]: max err {err:.3e}, bar {REL * scale:.3e}")
    assert err <= REL * scale


def test_17x17_image(C_):
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    ups = upstream(c.H, c.W, 13, c.ok)
    held(call(C_, g, cam, c.H, c.W, c.fout, ups), c.ref(ups), "17x17")


@pytest.mark.parametrize("name", sorted(ar.SMALL))
def test_small_models_on_a_17x19_image(C_, name):
    """P = 65 (one Gaussian past a wave: two blocks of the per-Gaussian kernel) and P = 1 on 17x19, partial tiles on both axes."""
    kw = ar.SMALL[name]
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    ups = upstream(c.H, c.W, 17, c.ok)
    held(call(C_, g, cam, c.H, c.W, c.fout, ups), c.ref(ups), name)


def test_portrait_camera_with_non_square_pixels(C_):
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", 600, ar.PORTRAIT["seed"])
    c = Case(C_, cam, g, cam.image_height, cam.image_width)
    ups = upstream(c.H, c.W, 14, c.ok)
    held(call(C_, g, cam, c.H, c.W, c.fout, ups), c.ref(ups), "portrait_far")


def stacked(P, W=32, H=32):
    """P faint Gaussians stacked over the first 16x16 tile of a 32x32 image: one list of more than 128 entries."""
    import synth_scene as ss
    cam = ss.make_camera(W, H, 30.0, 1)
    g = ss.make_gaussians(P, cam, seed=5, degree_mode="mixed", scale_mu=0.05)
    rng = np.random.default_rng(6)
    Vi = np.linalg.inv(np.asarray(cam.world_view_transform, np.float64).reshape(4, 4))
    fx = W / (2 * cam.tanfovx)
    zv = rng.uniform(2.0, 6.0, P)
    xv = (rng.uniform(3.0, 12.0, P) - (W - 1) / 2) / fx * zv
    yv = (rng.uniform(3.0, 12.0, P) - (H - 1) / 2) / (H / (2 * cam.tanfovy)) * zv
    g["means3D"] = (np.stack([xv, yv, zv, np.ones(P)], 1) @ Vi)[:, :3].astype(np.float32)
    g["scales"] = (0.02 * zv[:, None] * rng.uniform(0.6, 1.4, (P, 3))).astype(np.float32)
    g["opacity"] = rng.uniform(-4.2, -3.2, (P, 1)).astype(np.float32)   # sigmoid: 1.5 % .. 4 %, a deep walk
    return cam, g


@pytest.mark.parametrize("P", [512, 203])
def test_lists_longer_than_one_chunk(C_, P):
    """512 Gaussians over one tile: a list of more than 128 entries, three staged chunks walked backwards; 203: a walk whose
    last chunk is partial (the slot count is no multiple of 64)."""
    cam, g = stacked(P)
    c = Case(C_, cam, g, 32, 32)
    ex = C_.export_binning(P, c.fout[0], 32, 32, c.fout[3], c.fout[4], c.fout[5])
    lens = (ex["ranges"][:, 1] - ex["ranges"][:, 0]).cpu().numpy()
    deepest = int(ex["n_contrib"].max())
    print(f"[aux grad stacked {P}] heaviest list {lens.max()}, deepest contributor {deepest}")
    if P == 512:
        assert lens.max() > 128 and deepest > 128, "three chunks must be walked"
    else:
        assert lens.max() > 64 and lens.max() % 64 != 0 and deepest % 64 != 0
    ups = upstream(32, 32, 15, c.ok)
    held(call(C_, g, cam, 32, 32, c.fout, ups), c.ref(ups), f"stacked {P}")


def test_empty_model_and_all_culled(C_):
    H, W = 40, 56
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=64, W=W, H=H))
    empty = {k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()}
    fout = C_._forward_common(None, *forward_args(empty, cam, H, W), exact=True)
    got = call(C_, empty, cam, H, W, fout, upstream(H, W, 16))
    assert all(got[k].shape[0] == 0 for k in got)
    behind = dict(g)
    behind["means3D"] = g["means3D"].copy()
    behind["means3D"][:, 2] = -np.abs(g["means3D"][:, 2]) - 1.0
    fout = C_._forward_common(None, *forward_args(behind, cam, H, W), exact=True)
    assert int(fout[0]) == 0 and not fout[2].any()
    got = call(C_, behind, cam, H, W, fout, upstream(H, W, 16))
    for k, t in got.items():
        assert t.shape[0] == 64 and not t.any(), k


def test_each_output_alone_and_no_upstream(C_, scene_a):
    c = scene_a
    ups = upstream(c.H, c.W, 11, c.ok)
    full = call(C_, c.g, c.cam, c.H, c.W, c.fout, ups, want=C_.AUX_GRADS)
    assert float(full["cov3D"].abs().max()) > 0
    for k in C_.AUX_GRADS:
        one = call(C_, c.g, c.cam, c.H, c.W, c.fout, ups, want=(k,))
        assert set(one) == {k} and torch.equal(one[k], full[k]), k
    assert call(C_, c.g, c.cam, c.H, c.W, c.fout, ups, want=()) == {}   # no output asked for: nothing comes back
    none = call(C_, c.g, c.cam, c.H, c.W, c.fout, [None, None, None])
    assert all(not t.any() for t in none.values())


def test_determinism_and_untouched_state(C_, scene_a):
    """Two calls give the same bits; the blobs are byte-identical before and after; the colour backward afterwards is the one
    without this call."""
    import synth_scene as ss
    c = scene_a
    g, cam, H, W = c.g, c.cam, c.H, c.W
    args = forward_args(g, cam, H, W)
    (bg, m3, colors, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
    dl = dev(ss.upstream_grad(W, H, seed=3) * (W * H))
    ups = upstream(H, W, 17)

    def run(with_aux):
        C_.hint_next_forward(True)
        fout = C_._forward_common(None, *args, exact=True)
        R, _, radii, geom, binning, img = fout
        aux = None
        if with_aux:
            before = [t.clone() for t in (geom, binning, img)]
            aux = call(C_, g, cam, H, W, fout, ups, want=C_.AUX_GRADS)
            again = call(C_, g, cam, H, W, fout, ups, want=C_.AUX_GRADS)
            for k in aux:
                assert torch.equal(aux[k], again[k]), k
            for a, b in zip(before, (geom, binning, img)):
                assert torch.equal(a, b), "a state blob was written"
        return C_.rasterize_gaussians_backward(bg, m3, radii, colors, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom,
                                               R, binning, img, 0.0, False)
    plain, after = run(False), run(True)
    for k, (a, b) in enumerate(zip(plain, after)):
        assert torch.equal(a, b), k


def test_captured_launch_follows_the_upstream_buffer(C_, scene_a):
    c = scene_a
    first, second = upstream(c.H, c.W, 18), upstream(c.H, c.W, 19)
    R, _, radii, geom, binning, img = c.fout
    fixed = [dev(u) for u in first]
    model = [dev(c.g[k]) for k in ("means3D", "scales", "rotations")]
    vm, pm = dev(c.cam.world_view_transform), dev(c.cam.full_proj_transform)

    def go():
        return C_.aux_maps_backward(c.P, R, c.H, c.W, geom, binning, img, vm, pm, c.cam.tanfovx, c.cam.tanfovy, model[0], model[1],
                                    1.0, model[2], EMPTY, radii, *fixed)
    want_first = {k: v.clone() for k, v in go().items()}   # warm-up outside the capture (the workspace size is asked here)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = go()
    for ups in (second, first):
        for dst, src in zip(fixed, ups):
            dst.copy_(dev(src))
        graph.replay()
        torch.cuda.synchronize()
        direct = call(C_, c.g, c.cam, c.H, c.W, c.fout, ups)
        for k in direct:
            assert torch.equal(static[k], direct[k]), k
    for k in want_first:
        assert torch.equal(static[k], want_first[k]), k
    assert not torch.equal(call(C_, c.g, c.cam, c.H, c.W, c.fout, second)["means3D"], want_first["means3D"])


class Model:
    """The reference's GaussianModel, as far as render() looks at it."""

    def __init__(self, g):
        sh = dev(g["sh"])
        self._xyz = dev(g["means3D"]).requires_grad_(True)
        self._features_dc = sh[:, :1].contiguous().requires_grad_(True)
        self._features_rest = sh[:, 1:].contiguous().requires_grad_(True)
        self._opacity = dev(g["opacity"]).requires_grad_(True)
        self._scaling = dev(np.log(g["scales"]).astype(np.float32)).requires_grad_(True)
        self._rotation = dev(g["rotations"] * 1.3).requires_grad_(True)
        self._degrees, self.active_sh_degree, self.max_sh_degree = dev(g["degrees"]), 3, 3

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def grads_close(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        assert err <= REL * max(scale, 1e-30), (what, k, err, scale)


@pytest.mark.parametrize("route", ["fused", "python_sh"])
def test_through_render(C_, route):
    """(render.sum() + depth.sum()).backward() = the sum of the two separate backwards, on the raw-parameter route and on the
    route through GaussianRasterizer; aux_grad=False is today's result, maps detached."""
    import r3dgs_render
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    H, W = kw["H"], kw["W"]
    pc = Model(g)
    view = NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = dev(BG)
    def options():   # any option the fused path does not cover sends the call through GaussianRasterizer (built per call:
        if route == "python_sh":   # its graph is freed by each backward)
            return dict(override_color=torch.sigmoid(pc._features_dc[:, 0, :]))
        return dict(variable_sh_bands=False)
    assert r3dgs_render.fused_path_applies(pc, pipe, options().get("override_color")) == (route == "fused")

    def backward_of(loss_of, aux_grad):
        for t in pc.leaves():
            t.grad = None
        out = r3dgs_render.render(view, pc, pipe, bg, aux=MAPS, aux_grad=aux_grad, **options())
        loss_of(out).backward()
        vs = out["viewspace_points"].grad
        return [torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in pc.leaves()] + [vs.clone()], out

    wimg = dev(np.linspace(0.5, 1.5, 3 * H * W, dtype=np.float32).reshape(3, H, W))
    only_render, plain = backward_of(lambda o: (o["render"] * wimg).sum(), False)
    for k in MAPS:
        assert not plain[k].requires_grad and plain[k].grad_fn is None
    only_depth, out = backward_of(lambda o: o["depth"].sum() + 0.5 * o["alpha"].sum(), True)
    for k in MAPS:
        assert out[k].requires_grad and torch.equal(out[k], plain[k]), k
    assert torch.equal(out["render"], plain["render"])
    assert float(only_depth[0].abs().max()) > 0 and float(only_depth[4].abs().max()) > 0 and float(only_depth[-1].abs().max()) > 0
    both, _ = backward_of(lambda o: (o["render"] * wimg).sum() + o["depth"].sum() + 0.5 * o["alpha"].sum(), True)
    grads_close(both, [a + b for a, b in zip(only_render, only_depth)], route)
    # the VALUES that came through render: the library call over a forward of the same model, then torch's chain rule through
    # exp / normalize by hand -- a route that fed the function other scales, rotations or positions would differ here
    with torch.no_grad():
        scales, rotations = torch.exp(pc._scaling), torch.nn.functional.normalize(pc._rotation)
        fout = C_.rasterize_gaussian_params(bg, pc._xyz, pc._features_dc, pc._features_rest, pc._degrees, pc._opacity, pc._scaling,
                                            pc._rotation, 1.0, view.world_view_transform, view.full_proj_transform, cam.tanfovx,
                                            cam.tanfovy, H, W, view.camera_center, False, False, exact=True)
        ones = torch.ones(H * W, device="cuda")
        d = C_.aux_maps_backward(kw["P"], fout[0], H, W, fout[3], fout[4], fout[5], view.world_view_transform,
                                 view.full_proj_transform, cam.tanfovx, cam.tanfovy, pc._xyz, scales, 1.0, rotations, EMPTY, fout[2],
                                 ones, 0.5 * ones, None)
    leaf = pc._rotation.detach().clone().requires_grad_(True)
    drot, = torch.autograd.grad(torch.nn.functional.normalize(leaf), leaf, d["rotations"])
    zero = torch.zeros_like
    want = [d["means3D"], zero(pc._features_dc), zero(pc._features_rest), d["opacity"], d["scales"] * scales, drot, d["means2D"]]
    grads_close(only_depth, want, route + ", values")
    with pytest.raises(ValueError, match="no_grad"), torch.no_grad():
        r3dgs_render.render(view, pc, pipe, bg, aux=MAPS, aux_grad=True, **options())


def test_through_render_quantised_and_refusals(C_):
    import r3dgs_render
    from tests import test_quantised_gpu as tq
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    import copy
    qm = copy.copy(tq.model("37-0-150-70")[0])   # the module's model is shared: requires_grad_ below rebinds this copy's tensors only
    c = tq.camera("131x77")
    qview = NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm, full_proj_transform=c.pm,
               camera_center=c.cp)
    with pytest.raises(ValueError, match="trainable"):
        r3dgs_render.render(qview, qm, pipe, c.bg, aux=MAPS, aux_grad=True)
    qm.requires_grad_(True)
    leaves = [t for t in (qm.codebooks, qm.xyz_master) if t is not None and t.requires_grad]
    assert leaves

    def backward_of(loss_of):
        for t in leaves:
            t.grad = None
        out = r3dgs_render.render(qview, qm, pipe, c.bg, aux=MAPS, aux_grad=True)
        loss_of(out).backward()
        return [t.grad.clone() for t in leaves] + [out["viewspace_points"].grad.clone()], out
    a, out = backward_of(lambda o: o["render"].sum())
    assert out["depth"].requires_grad
    b, _ = backward_of(lambda o: o["depth"].sum())
    assert float(b[0].abs().max()) > 0
    both, _ = backward_of(lambda o: o["render"].sum() + o["depth"].sum())
    grads_close(both, [x + y for x, y in zip(a, b)], "quantised")
    # the values: the library call over the quantised forward's state, then autograd through this test's own decode
    xyz, _, _, opacity, scaling, rotation, _ = qm.decode_for_training()
    scales, rotations = torch.exp(scaling), torch.nn.functional.normalize(rotation)
    fout = tq.quantised_forward(C_, tq.model("37-0-150-70")[0], c)
    with torch.no_grad():
        d = C_.aux_maps_backward(qm.P, fout[0], c.H, c.W, fout[3], fout[4], fout[5], c.vm, c.pm, c.tanfovx, c.tanfovy, xyz, scales,
                                 1.0, rotations, EMPTY, fout[2], torch.ones(c.H * c.W, device="cuda"), None, None)
    want = torch.autograd.grad([xyz * 1.0, opacity, scales, rotations], leaves,
                               [d["means3D"], d["opacity"], d["scales"], d["rotations"]], allow_unused=True)
    grads_close(b, [torch.zeros_like(t) if w is None else w for w, t in zip(want, leaves)] + [d["means2D"]], "quantised, values")


def test_empty_model_through_render(C_):
    """aux_grad=True on a model without Gaussians: zero maps that are attached (a backward through them is valid)."""
    import r3dgs_render
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=8))
    pc = Model({k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()})
    view = NS(image_height=40, image_width=56, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))
    out = r3dgs_render.render(view, pc, NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False), dev(BG), aux=MAPS,
                              aux_grad=True)
    for k in MAPS:
        assert out[k].shape == (1, 40, 56) and out[k].requires_grad and not out[k].any(), k
    out["depth"].sum().backward()
    assert pc._xyz.grad is None or pc._xyz.grad.shape == (0, 3)


def test_precomputed_covariance(C_):
    """cov3D_precomp instead of scales and rotations: dL_dcov3D and the other gradients against the float64 reference."""
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
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
    ups = upstream(c.H, c.W, 21, c.ok)
    R, _, radii, geom, binning, img = fout
    got = C_.aux_maps_backward(c.P, R, c.H, c.W, geom, binning, img, dev(cam.world_view_transform), dev(cam.full_proj_transform),
                               cam.tanfovx, cam.tanfovy, dev(g["means3D"]), EMPTY, 1.0, EMPTY, dev(cov), radii, *[dev(u) for u in ups],
                               want=C_.AUX_GRADS)
    ref = agr.reference_grads(c.st, g["means3D"], g["opacity"], None, None, cam.world_view_transform, cam.full_proj_transform,
                              cam.tanfovx, cam.tanfovy, *ups, cov3D_precomp=cov)
    assert not got["scales"].any() and not got["rotations"].any()
    for k in ("means2D", "means3D", "opacity", "cov3D"):
        a, b = got[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        a = a[:, :2] if k == "means2D" else a
        scale, err = np.abs(b).max(), np.abs(a - b.reshape(a.shape)).max()
        print(f"[aux grad cov3D_precomp] {k}: max err {err:.3e}, bar {REL * scale:.3e}")
        assert scale > 0 and err <= REL * scale, (k, err, scale)
