"""GPU tests (-m gpu) of the maps' share of a camera gradient: render(camera_grad_maps=True) end to end against the float64
reference tests/camera_maps_ref.py, the cross-check against the colour route on override_color = (z, 1, 0), the _screen entry
points against their siblings, a frozen model, the camera pass alone at sizes that make lanes take several trips and at
unaligned ones, determinism and a captured launch, the empty cases, and that nothing else moved.

Bar, per tensor (the project's gradient bar): max |got - ref| <= 1e-4 * max |ref|.  The masked pixels -- the oracle's
threshold-ambiguous ones and aux_ref's median-near-0.5 ones (tests/test_camera_maps_cpu.py measures their share) -- carry a
zero upstream gradient on both sides.  The fp32 forward state alone is worth cms.STATE_ROUNDING of a tensor's largest entry
(measured on the CPU, tests/test_camera_maps_cpu.py reproduces it): under a quarter of the bar, so the end-to-end bar is the
project's 1e-4 itself.  The float64 pose-recovery loop reaches cms.POSE_RATIO_FP64; the GPU run must reach within a factor of two
of it, the margin tests/test_camera_grad_gpu.py gives its own float64 figure.  Measured worst values:
profiles/camera_maps_gpu_tests.txt."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import camera_grad_scenes as cs
from tests import camera_maps_ref as cmr
from tests import camera_maps_scenes as cms
from tests import test_camera_grad_gpu as tcg
from tests import test_camera_maps_cpu as tcpu

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
REL = 1e-4
PIPE = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
NEAR_FAR = (0.5, 50.0)
dev = tcg.dev


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


class Case(tcg.Scene):
    """tcg.Scene plus the oracle's state over the device's own rects, the unmasked pixels and seeded upstream gradients."""

    def __init__(self, C_, cam, g):
        super().__init__(cam, g)
        H, W = self.H, self.W
        d = self.d
        self.fout = C_._forward_common(None, self.bg, d["means3D"], EMPTY, d["opacity"], d["scales"], d["rotations"], 1.0, EMPTY,
                                       self.vm, self.pm, cam.tanfovx, cam.tanfovy, H, W, d["sh"], d["degrees"], self.cp, False,
                                       False, exact=True)
        ref = cs.oracle_forward(cam, g)
        if C_.tight_rects():
            rects = C_.export_rects(self.P, self.fout[3]).cpu().numpy()
            rects[ref["radii"] <= 0] = 0
            ref = orc.with_rects(ref, rects, want_ambig=True)
        self.st, self.radii_np = ref["state"], ref["radii"]
        masked = (ref["ambig"].reshape(-1) != 0) | ar.aux_ref(self.st)["median_ambig"].reshape(-1)
        self.ok = (~masked).astype(np.float32)
        rng = np.random.default_rng(17)
        u = lambda *shape: (rng.uniform(-1.0, 1.0, shape) * self.ok).astype(np.float32)   # noqa: E731
        self.F = rng.uniform(-1.0, 1.0, (self.P, 5)).astype(np.float32)
        self.ups = dict(depth=u(H * W), alpha=u(H * W), median_depth=u(H * W), dist=u(H * W), feat=u(5, H * W),
                        colour=self.dl_np.reshape(3, -1) * self.ok)
        self._refs = {}

    def up_of(self, which):
        """The reference's `up` dictionary of a configuration name."""
        a = {k: self.ups[k] for k in ("depth", "alpha", "median_depth")}
        return dict(aux=a, dist_lin=dict(distortion=(self.ups["dist"], 0.0, 0.0)), dist_nf=dict(distortion=(self.ups["dist"], *NEAR_FAR)),
                    feat=dict(features=(self.F, self.ups["feat"])),
                    depth_alpha=dict(depth=self.ups["depth"], alpha=self.ups["alpha"]))[which]

    def ref(self, which):
        if which not in self._refs:   # computed once per configuration, shared, never modified
            self._refs[which] = cmr.camera_grads(self.st, self.g, self.cam, self.up_of(which))
        return self._refs[which]


@pytest.fixture(scope="module")
def cases(C_):
    return {"k64": Case(C_, *cms.kernel_scene(64)), "k3001": Case(C_, *cms.kernel_scene(3001)), "portrait": Case(C_, *cms.portrait_scene())}


def render_with(c, which, view, pc, colour=False, **kw):
    """render() with the maps of configuration `which` -> (out, the loss sum(g * map) [+ the colour loss])."""
    import r3dgs_render
    kwargs = dict(kw)
    if which in ("aux", "depth_alpha", "all"):
        kwargs.update(aux=("depth", "alpha", "median_depth") if which != "depth_alpha" else ("depth", "alpha"), aux_grad=True)
    if which in ("dist_lin", "all"):
        kwargs.update(distortion=True)
    if which == "dist_nf":
        kwargs.update(distortion=NEAR_FAR)
    if which in ("feat", "all"):
        kwargs.update(features=dev(c.F), features_geom_grad=True)
    out = r3dgs_render.render(view, pc, PIPE, c.bg, **kwargs)
    loss = 0.0
    for k in ("depth", "alpha", "median_depth"):
        if k in out:
            loss = loss + (out[k].reshape(-1) * dev(c.ups[k])).sum()
    if "distortion" in out:
        loss = loss + (out["distortion"].reshape(-1) * dev(c.ups["dist"])).sum()
    if "features" in out:
        loss = loss + (out["features"].reshape(5, -1) * dev(c.ups["feat"])).sum()
    if colour:
        loss = loss + (out["render"].reshape(3, -1) * dev(c.ups["colour"].astype(np.float32))).sum()
    return out, loss


def held(got, ref, what, bar=REL):
    scale = np.abs(ref).max()
    err = np.abs(got.detach().double().cpu().numpy().reshape(ref.shape) - ref).max()
    print(f"[camera maps {what}] max err {err:.3e}, bar {bar * scale:.3e} ({err / scale if scale else 0.0:.2e} of max |ref| {scale:.3e})")
    assert scale > 0 and err <= bar * scale, (what, err, scale)
    return err / scale


@pytest.mark.parametrize("name", ["k64", "k3001", "portrait"])
@pytest.mark.parametrize("which", ["aux", "dist_lin", "dist_nf", "feat"])
def test_each_map_alone_through_render(C_, cases, name, which):
    """dL_dviewmatrix and dL_dprojmatrix of a loss on one map, model trainable, against the float64 reference."""
    assert cms.STATE_ROUNDING <= REL / 4   # what the fp32 state alone is worth leaves the bar its room
    c = cases[name]
    view, pc = tcg.view_of(c, True), tcg.Model(c)
    _, loss = render_with(c, which, view, pc, camera_grad_maps=True)
    loss.backward()
    ref = c.ref(which)
    held(view.world_view_transform.grad, ref["viewmatrix"], f"{name} {which} viewmatrix")
    held(view.full_proj_transform.grad, ref["projmatrix"], f"{name} {which} projmatrix")
    assert not view.world_view_transform.grad[:, 3].any() and not view.full_proj_transform.grad[:, 2].any()
    assert view.camera_center.grad is None


def test_all_maps_with_a_colour_loss_and_nothing_else_moved(C_, cases):
    """Every map and the colour image in one loss: the camera gradient is the colour route's share plus the maps' (the
    reference's, summed); and with the keyword on, the image, the radii, every model gradient and the colour route's own camera
    share are the keyword-off values bit for bit."""
    import r3dgs_render
    c = cases["k3001"]
    view, pc = tcg.view_of(c, True), tcg.Model(c)
    out, loss = render_with(c, "all", view, pc, colour=True, camera_grad_maps=True)
    loss.backward()
    # the colour route alone, camera differentiable; the maps, camera detached: the keyword-off values
    v2, pc2 = tcg.view_of(c, True), tcg.Model(c)
    o2 = r3dgs_render.render(v2, pc2, PIPE, c.bg)
    (o2["render"].reshape(3, -1) * dev(c.ups["colour"].astype(np.float32))).sum().backward()
    v3, pc3 = tcg.view_of(c, False), tcg.Model(c)
    o3, l3 = render_with(c, "all", v3, pc3, colour=True)
    l3.backward()
    assert torch.equal(out["render"], o3["render"]) and torch.equal(out["radii"], o3["radii"]) and torch.equal(out["render"], o2["render"])
    for a, b in zip(pc.leaves(), pc3.leaves()):
        assert torch.equal(a.grad, b.grad)
    assert torch.equal(out["viewspace_points"].grad, o3["viewspace_points"].grad)
    assert torch.equal(view.camera_center.grad, v2.camera_center.grad)
    maps_ref = {k: sum(c.ref(w)[k] for w in ("aux", "dist_lin", "feat")) for k in ("viewmatrix", "projmatrix")}
    for k, t, t2 in (("viewmatrix", view.world_view_transform, v2.world_view_transform),
                     ("projmatrix", view.full_proj_transform, v2.full_proj_transform)):
        share = t.grad.double() - t2.grad.double()   # the maps' three shares as autograd added them to the colour route's
        scale = np.abs(maps_ref[k]).max()
        err = np.abs(share.cpu().numpy() - maps_ref[k]).max()
        print(f"[camera maps all + colour] {k}: max err {err:.3e}, bar {REL * scale:.3e} (colour share max {float(t2.grad.abs().max()):.3e})")
        assert err <= REL * scale


def test_depth_alpha_share_is_the_colour_route_on_z_1_0(C_, cases):
    """Without the reference: the depth + alpha share equals the colour route's camera gradient of a second render with
    override_color = stack(z(V), 1, 0) built in torch from the same camera, over black."""
    import r3dgs_render
    c = cases["k3001"]
    view, pc = tcg.view_of(c, True), tcg.Model(c)
    _, loss = render_with(c, "depth_alpha", view, pc, camera_grad_maps=True)
    loss.backward()
    v2, pc2 = tcg.view_of(c, True), tcg.Model(c)
    ones = torch.ones(c.P, 1, device="cuda")
    z = (torch.cat([pc2._xyz.detach(), ones], 1) @ v2.world_view_transform)[:, 2:3]
    colours = torch.cat([z, ones, torch.zeros_like(ones)], 1)
    out = r3dgs_render.render(v2, pc2, PIPE, torch.zeros(3, device="cuda"), override_color=colours)
    img = out["render"].reshape(3, -1)
    (img[0] * dev(c.ups["depth"]) + img[1] * dev(c.ups["alpha"])).sum().backward()
    for k, a, b in (("viewmatrix", view.world_view_transform.grad, v2.world_view_transform.grad),
                    ("projmatrix", view.full_proj_transform.grad, v2.full_proj_transform.grad)):
        held(a, b.double().cpu().numpy(), f"depth + alpha against override_color, {k}")


def model_args(c):
    d = c.d
    return (c.vm, c.pm, c.cam.tanfovx, c.cam.tanfovy, d["means3D"], d["scales"], 1.0, d["rotations"], EMPTY, c.fout[2])


def screen_pair(C_, c, which, want_model=True):
    """(the sibling's result, the _screen form's) of one map backward over the case's exact forward."""
    R, _, radii, geom, binning, img = c.fout
    head = (c.P, R, c.H, c.W, geom, binning, img) + model_args(c)
    want = C_.AUX_GRADS if want_model else ("means2D",)
    if which == "aux":
        tail = tuple(dev(c.ups[k]) for k in ("depth", "alpha", "median_depth"))
        return (C_.aux_maps_backward(*head, *tail, want=want), C_.aux_maps_backward_screen(*head, *tail, want=want + C_.SCREEN_GRADS))
    if which in ("dist_lin", "dist_nf"):
        nf = NEAR_FAR if which == "dist_nf" else (0.0, 0.0)
        _, mom = C_.distortion_map(c.P, R, c.H, c.W, geom, binning, img, *nf, want_moments=True)
        tail = (dev(c.ups["dist"]), mom) + nf
        return (C_.distortion_map_backward(*head, *tail, want=want), C_.distortion_backward_screen(*head, *tail, want=want + C_.SCREEN_GRADS))
    tail = (dev(c.F), dev(c.ups["feat"]))
    return (C_.feature_maps_backward(*head, *tail, want=want), C_.feature_maps_backward_screen(*head, *tail, want=want + C_.SCREEN_GRADS))


@pytest.mark.parametrize("which", ["aux", "dist_lin", "dist_nf", "feat"])
def test_screen_entry_points_against_their_siblings(C_, cases, which):
    """The six shared outputs bit for bit (both settings of set_f64_chain), dL_dconic and dL_dz within 1e-4 of the reference's
    conic and z gradients, zero rows for culled Gaussians, and the frozen-model form the same screen-space bits."""
    c = cases["k3001"]
    ref = c.ref(which)
    was = C_.set_f64_chain(True)
    try:
        for f64 in (True, False):
            C_.set_f64_chain(f64)
            sib, scr = screen_pair(C_, c, which)
            for k in C_.AUX_GRADS:
                assert torch.equal(sib[k], scr[k]), (which, k, f64)
    finally:
        C_.set_f64_chain(was)
    culled = c.fout[2] <= 0
    assert int(culled.sum()) > 0 and not scr["conic"][culled].any() and not scr["z"][culled].any() and not scr["conic"][:, 2].any()
    held(scr["conic"][:, [0, 1, 3]], ref["conic"], f"{which} dL_dconic")
    if which == "feat":
        assert not scr["z"].any() and not ref["z"].any()
    else:
        held(scr["z"].reshape(-1), ref["z"], f"{which} dL_dz")
    _, frozen = screen_pair(C_, c, which, want_model=False)
    for k in ("means2D", "conic", "z"):
        assert torch.equal(frozen[k], scr[k]), (which, k)


@pytest.mark.parametrize("C_feat", [17, 40])
def test_feature_screen_entry_point_over_several_channel_groups(C_, cases, C_feat):
    """More than 16 channels: the geometric slab holds 4 * groups rows per list slot (2 and 3 groups here), which the shared
    per-Gaussian kernel of the _screen form walks in the sibling's order: the seven shared outputs bit for bit, dL_dz zero."""
    c = cases["k3001"]
    rng = np.random.default_rng(5)
    F = dev(rng.uniform(-1.0, 1.0, (c.P, C_feat)).astype(np.float32))
    gout = dev((rng.uniform(-1.0, 1.0, (C_feat, c.H * c.W)) * c.ok).astype(np.float32))
    R, _, radii, geom, binning, img = c.fout
    head = (c.P, R, c.H, c.W, geom, binning, img) + model_args(c)
    sib = C_.feature_maps_backward(*head, F, gout)
    scr = C_.feature_maps_backward_screen(*head, F, gout, want=C_.FEATURE_GRADS + C_.SCREEN_GRADS)
    for k in C_.FEATURE_GRADS:
        assert torch.equal(sib[k], scr[k]), k
    assert float(scr["conic"].abs().max()) > 0 and not scr["z"].any()
    frozen = C_.feature_maps_backward_screen(*head, F, gout, want=("means2D",) + C_.SCREEN_GRADS)
    for k in ("means2D", "conic", "z"):
        assert torch.equal(frozen[k], scr[k]), k


def test_pose_recovery_from_depth_and_alpha(C_):
    """A tracker on cs.pose_target_and_start(): ~400 frozen Gaussians at 64x48, target depth and alpha maps rendered at the true
    pose, the camera started a few hundredths of a radian and of a scene unit off, POSE_STEPS Adam steps at POSE_LR on
    RefinedCamera.xi through render(aux_grad=True, camera_grad_maps=True) with a depth + alpha loss only (no colour).  The same
    loop in float64 through the reference reaches cms.POSE_RATIO_FP64 (tests/test_camera_maps_cpu.py); the fp32 and float64
    trajectories differ, so the GPU run must reach within a factor of two of it -- the margin of tcg.test_pose_recovery -- and
    the pose error must end below where it started."""
    import r3dgs_render
    from r3dgs_camera import RefinedCamera
    cam, g, true, start = cs.pose_target_and_start()
    s = tcg.Scene(cam, g)
    pc = tcg.Model(s)
    for t in pc.leaves():
        t.requires_grad_(False)
    with torch.no_grad():
        target = r3dgs_render.render(tcg.view_of(s, False), pc, PIPE, s.bg, aux=("depth", "alpha"))
    begin = NS(image_height=s.H, image_width=s.W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=start.astype(np.float32),
               projection_matrix=cam.projection_matrix)
    rc = RefinedCamera(begin, device="cuda")
    opt = torch.optim.Adam([rc.xi], lr=cs.POSE_LR)
    err0 = rc.pose_error(true)
    losses = []
    for _ in range(cs.POSE_STEPS + 1):
        out = r3dgs_render.render(rc, pc, PIPE, s.bg, aux=("depth", "alpha"), aux_grad=True, camera_grad_maps=True)
        loss = (out["depth"] - target["depth"]).abs().mean() + (out["alpha"] - target["alpha"]).abs().mean()
        losses.append(loss)
        if len(losses) > cs.POSE_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    losses = [float(v.detach()) for v in losses]
    ratio, err1 = losses[-1] / losses[0], rc.pose_error(true)
    print(f"[camera maps pose] loss {losses[0]:.4e} -> {losses[-1]:.4e}, ratio {ratio:.3f} (fp64: {cms.POSE_RATIO_FP64:.4f}); "
          f"pose error {err0} -> {err1}")
    assert all(t.grad is None for t in pc.leaves())
    assert ratio <= 2 * cms.POSE_RATIO_FP64
    assert err1[0] < err0[0] and err1[1] < err0[1]


def test_frozen_model_only_the_pose_gets_a_gradient(C_, cases):
    """A tracker: RefinedCamera, nothing of the model trainable, colour + depth + alpha loss.  Only cam.xi gets a gradient, and
    it is the trainable-model run's bit for bit."""
    from r3dgs_camera import RefinedCamera
    c = cases["k64"]
    grads = []
    for trainable in (True, False):
        rc = RefinedCamera(c.cam, device="cuda")
        pc = tcg.Model(c)
        if not trainable:
            for t in pc.leaves():
                t.requires_grad_(False)
        _, loss = render_with(c, "depth_alpha", rc, pc, colour=True, camera_grad_maps=True)
        loss.backward()
        assert rc.xi.grad is not None and float(rc.xi.grad.abs().max()) > 0
        if not trainable:
            assert all(t.grad is None for t in pc.leaves())
        grads.append(rc.xi.grad.clone())
    assert torch.equal(grads[0], grads[1])


def random_inputs(P, visible, seed=0):
    rng = np.random.default_rng(seed)
    cam, _ = cs.kernel_scene(64)
    t = rng.uniform(-1.0, 1.0, (P, 3)) * np.array([1.5, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0]) * rng.uniform(2.0, 8.0, (P, 1))
    R, tr_ = cam.world_view_transform[:3, :3].astype(np.float64), cam.world_view_transform[3, :3].astype(np.float64)
    g = dict(means3D=((t - tr_) @ np.linalg.inv(R)).astype(np.float32), scales=rng.uniform(0.02, 0.3, (P, 3)).astype(np.float32))
    q = rng.normal(size=(P, 4))
    g["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    radii = (rng.uniform(size=P) < visible).astype(np.int32) * 5
    return cam, g, radii, rng.normal(size=(P, 2)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32), \
        rng.normal(size=P).astype(np.float32)


def pass_inputs(cam, g, radii, g2, gcon, gz):
    """The arguments of C_.camera_backward_maps on the device (a None gradient input stays None)."""
    P = len(radii)
    g2d = None if g2 is None else dev(np.concatenate([g2, np.zeros((P, 1), np.float32)], 1))
    gcd = None if gcon is None else dev(np.stack([gcon[:, 0], gcon[:, 1], np.zeros(P, np.float32), gcon[:, 2]], 1))
    return (dev(g["means3D"]), dev(g["scales"]), dev(g["rotations"]), 1.0, None, dev(cam.world_view_transform),
            dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, dev(radii), g2d, gcd,
            None if gz is None else dev(gz))


def camera_pass(C_, cam, g, radii, g2, gcon, gz, **kw):
    return C_.camera_backward_maps(*pass_inputs(cam, g, radii, g2, gcon, gz), **kw)


@pytest.mark.parametrize("P,visible", [(140_000, 0.1), (37, 0.7), (64, 0.7)])
def test_the_camera_pass_alone(C_, P, visible):
    """Random per-Gaussian inputs, mostly culled radii at P = 140 000 (beyond the 512 x 256 row cap: lanes take several trips),
    one partial wave and one full one: against the host function summed in float64 in index order, to 1e-9 of the sum of the
    absolute shares (plus the fp32 rounding of the output itself).  Both settings of set_f64_chain."""
    from tests.hostcheck_build import EXACT, build_shim
    here = os.path.dirname(os.path.abspath(__file__))
    shim = build_shim(os.path.join(here, "hostcheck_camera_maps", "hostcheck_camera_maps.hip"),
                      os.path.join(here, "hostcheck_camera_maps", "libhostcheck_camera_maps.so"), EXACT, None)
    cam, g, radii, g2, gcon, gz = random_inputs(P, visible)
    was = C_.set_f64_chain(True)
    try:
        for f64 in (True, False):
            C_.set_f64_chain(f64)
            got = camera_pass(C_, cam, g, radii, g2, gcon, gz)
            _, _, sums, abs_sums = tcpu.run_shim(shim, cam, g, radii, g2, gcon, gz, f64=f64)
            for k, want, scale in zip(("viewmatrix", "projmatrix"), tcpu.sums_as_matrices(sums), tcpu.sums_as_matrices(abs_sums)):
                a = got[k].double().cpu().numpy()
                bar = 1e-9 * scale + np.abs(want) * 2.0 ** -24
                worst = (np.abs(a - want) / np.maximum(bar, 1e-300)).max()
                print(f"[camera maps pass alone P={P} f64={f64}] {k}: worst error / bar {worst:.3f}")
                assert (np.abs(a - want) <= bar).all() and np.abs(want).max() > 0
    finally:
        C_.set_f64_chain(was)


def test_determinism_capture_and_null_inputs(C_):
    cam, g, radii, g2, gcon, gz = random_inputs(3001, 0.6, seed=1)
    a, b = camera_pass(C_, cam, g, radii, g2, gcon, gz), camera_pass(C_, cam, g, radii, g2, gcon, gz)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # NULL gradient inputs are zeros; the pass is linear in its three inputs
    z2, zc, zz = np.zeros_like(g2), np.zeros_like(gcon), np.zeros_like(gz)
    for nulls, zeros in (((None, gcon, gz), (z2, gcon, gz)), ((g2, None, gz), (g2, zc, gz)), ((g2, gcon, None), (g2, gcon, zz))):
        x, y = camera_pass(C_, cam, g, radii, *nulls), camera_pass(C_, cam, g, radii, *zeros)
        assert all(torch.equal(x[k], y[k]) for k in x)
    none = camera_pass(C_, cam, g, radii, None, None, None)
    assert not none["viewmatrix"].any() and not none["projmatrix"].any()
    only = camera_pass(C_, cam, g, radii, g2, gcon, gz, want=("projmatrix",))
    assert list(only) == ["projmatrix"] and torch.equal(only["projmatrix"], a["projmatrix"])
    # a captured launch replays to the eager bits (inputs on the device and the workspace sized outside the capture: same P)
    inputs = pass_inputs(cam, g, radii, g2, gcon, gz)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        C_.camera_backward_maps(*inputs)   # warm-up on the capture stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            cap = C_.camera_backward_maps(*inputs)
    for t in cap.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(cap[k], a[k]) for k in a)


def test_empty_model_and_all_culled(C_):
    cam, g, radii, g2, gcon, gz = random_inputs(64, 0.7)
    got = camera_pass(C_, cam, g, np.zeros_like(radii), g2, gcon, gz)
    assert not got["viewmatrix"].any() and not got["projmatrix"].any()
    z = lambda *shape, **kw: torch.zeros(*shape, device="cuda", **kw)   # noqa: E731
    got = C_.camera_backward_maps(z(0, 3), z(0, 3), z(0, 4), 1.0, None, dev(cam.world_view_transform), dev(cam.full_proj_transform),
                                  cam.tanfovx, cam.tanfovy, 64, 96, z(0, dtype=torch.int32), z(0, 3), z(0, 4), z(0))
    assert tuple(got["viewmatrix"].shape) == (4, 4) and not got["viewmatrix"].any() and not got["projmatrix"].any()
