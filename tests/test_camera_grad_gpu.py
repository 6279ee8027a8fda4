"""GPU tests (-m gpu) of the camera gradients (include/r3dgs_camera.h r3dgs_camera_backward, csrc/camera_bwd.hip): the kernel
alone against the float64 reference tests/camera_grad_ref.py, end to end against fp64 autograd of oracle/torch_ref.render, the
gauge identity at a size the autograd reference cannot reach, nothing else moved, determinism and a captured launch, the edge
cases, and pose recovery through r3dgs_camera.RefinedCamera.

Bar, per tensor (the project's gradient bar): max |got - ref| <= 1e-4 * max |ref|.  The oracle's threshold-ambiguous pixels (at
most 0.1 % of each scene: tests/test_camera_grad_cpu.py) carry a zero upstream gradient on both sides."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr
from tests import camera_grad_ref as cgr
from tests import camera_grad_scenes as cs

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
REL = 1e-4
NAMES = ("viewmatrix", "projmatrix", "campos")
# measured on the CPU and written once in tests/camera_grad_scenes.py (tests/test_camera_grad_cpu.py reproduces each figure):
# the fp32 forward state alone is worth cs.STATE_ROUNDING for the 35 sums -- under a quarter of REL, so the end-to-end bar is REL
# itself; the CPU oracle's own gradients satisfy the gauge identity to cs.GAUGE_RESIDUAL, the product is allowed four times that;
# the fp64 pose-recovery loop reaches cs.POSE_RATIO_FP64, the GPU run must reach within a factor of two of it.
GAUGE_TOLERANCE = 4 * cs.GAUGE_RESIDUAL

T = lambda a: torch.tensor(np.asarray(a, np.float64))   # noqa: E731
f32 = lambda v: float(np.float32(v))                    # noqa: E731


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


def dev(a):
    return EMPTY if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Scene:
    """A scene on the device, the oracle's ambiguous pixels and a seeded upstream gradient that is zero on them."""

    def __init__(self, cam, g, seed=5):
        self.cam, self.g, self.P = cam, g, len(g["means3D"])
        self.H, self.W = cam.image_height, cam.image_width
        out = cs.oracle_forward(cam, g)
        assert (out["ambig"] != 0).mean() <= 1e-3
        self.cov3D = out["state"]["cov3D"]
        self.dl_np = cs.upstream(cam, out["ambig"], seed)
        self.dl = dev(self.dl_np)
        self.d = {k: dev(v) for k, v in g.items()}
        self.vm, self.pm, self.cp = dev(cam.world_view_transform), dev(cam.full_proj_transform), dev(cam.camera_center)
        self.bg = dev(cs.BG)
        sh = self.d["sh"]
        self.dc, self.rest = sh[:, :1].contiguous(), sh[:, 1:].contiguous()
        self.raw_scaling = dev(np.log(g["scales"]).astype(np.float32))
        self.raw_rotation = dev((g["rotations"] * np.linspace(0.5, 2.0, self.P)[:, None]).astype(np.float32))

    def settings(self, dgr, vm=None, pm=None, cp=None):
        return dgr.GaussianRasterizationSettings(
            image_height=self.H, image_width=self.W, tanfovx=self.cam.tanfovx, tanfovy=self.cam.tanfovy, bg=self.bg, scale_modifier=1.0,
            viewmatrix=self.vm if vm is None else vm, projmatrix=self.pm if pm is None else pm, sh_degree=3,
            campos=self.cp if cp is None else cp, prefiltered=False, debug=False)


@pytest.fixture(scope="module")
def kernel_scenes():
    return {P: Scene(*cs.kernel_scene(P)) for P in cs.KERNEL_SIZES}


def operator_alone(C_, s, mode):
    """Forward, the library's own backward (asked for dL_dconic as well), then the operator -> (got, the sums, radii)."""
    cam, d = s.cam, s.d
    cov = dev(s.cov3D) if mode == "cov3D_precomp" else EMPTY
    sc, rot = (EMPTY, EMPTY) if mode == "cov3D_precomp" else (d["scales"], d["rotations"])
    if mode == "raw":
        fout = C_.rasterize_gaussian_params(s.bg, d["means3D"], s.dc, s.rest, d["degrees"], d["opacity"], s.raw_scaling, s.raw_rotation,
                                            1.0, s.vm, s.pm, cam.tanfovx, cam.tanfovy, s.H, s.W, s.cp, False, False, exact=True)
        R, _, radii, geom, binning, img = fout
        back = C_.rasterize_gaussian_params_backward(s.bg, d["means3D"], radii, s.dc, s.rest, d["degrees"], d["opacity"], s.raw_scaling,
                                                     s.raw_rotation, 1.0, s.vm, s.pm, cam.tanfovx, cam.tanfovy, s.dl, s.cp, geom, R,
                                                     binning, img, 0.0, False, _want_2d=True)
        g2, gcol, gcon = back[0], back[7], back[8]
        got = C_.camera_backward(d["means3D"], d["degrees"], s.dc, s.rest, s.raw_scaling, s.raw_rotation, 1.0, None, True, s.vm, s.pm,
                                 s.cp, cam.tanfovx, cam.tanfovy, s.H, s.W, radii, geom, g2, gcon, gcol)
    else:
        if mode == "no_cache":
            C_.hint_next_forward(False)   # r3dgs_forward_hint(0): a lean geometry blob, no SH direction derivatives in it
        fout = C_._forward_common(None, s.bg, d["means3D"], EMPTY, d["opacity"], sc, rot, 1.0, cov, s.vm, s.pm, cam.tanfovx,
                                  cam.tanfovy, s.H, s.W, d["sh"], d["degrees"], s.cp, False, False, exact=True)
        R, _, radii, geom, binning, img = fout
        back = C_.rasterize_gaussians_backward(s.bg, d["means3D"], radii, EMPTY, sc, rot, 1.0, cov, s.vm, s.pm, cam.tanfovx,
                                               cam.tanfovy, s.dl, d["sh"], d["degrees"], s.cp, geom, R, binning, img, 0.0, False,
                                               _want_conic=True)
        g2, gcol, gcon = back[0], back[1], back[8]
        got = C_.camera_backward(d["means3D"], d["degrees"], d["sh"], None, sc, rot, 1.0, cov, False, s.vm, s.pm, s.cp, cam.tanfovx,
                                 cam.tanfovy, s.H, s.W, radii, geom, g2, gcon, gcol)
    assert sh_cache_word(geom) == (0 if mode == "no_cache" else 1), mode   # which branch of camera_grad_kernel this mode takes
    assert (geom.numel() == C_._blob_bytes("geom_lean", s.P)) == (mode == "no_cache"), mode
    return got, (g2, gcon, gcol), radii


def sh_cache_word(geom):
    """GeomHeader::sh_cache of a geometry blob: word 9 of the header, which sits at the blob's first 256-byte boundary."""
    first = (-geom.data_ptr()) % 256
    return int(geom[first:first + 256].view(torch.int32)[9])


def reference_of(s, sums, radii, raw=False):
    g, cam = s.g, s.cam
    g2, gcon, gcol = (t.cpu().numpy() for t in sums)
    if raw:   # the activations the kernel applies, in float64 from the raw tensors
        q = s.raw_rotation.cpu().numpy().astype(np.float64)
        cov = cgr.cov3d_of(np.exp(s.raw_scaling.cpu().numpy().astype(np.float64)), q / np.linalg.norm(q, axis=1, keepdims=True))
    else:
        cov = s.cov3D
    return cgr.camera_grads(g["means3D"], cov, g["sh"], g["degrees"], radii.cpu().numpy(), cam.world_view_transform,
                            cam.full_proj_transform, cam.camera_center, s.W, s.H, f32(cam.tanfovx), f32(cam.tanfovy), g2, gcon, gcol)


def held(got, ref, what, bar=REL):
    for k in NAMES:
        a, b = got[k].detach().cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        scale, err = np.abs(b).max(), np.abs(a - b.reshape(a.shape)).max()
        print(f"[camera grad {what}] {k}: max err {err:.3e} = {err / scale:.2e} of max |ref| {scale:.3e} (bar {bar:.1e})")
        assert scale > 0 and err <= bar * scale, (what, k, err, scale)
    assert not got["viewmatrix"][:, 3].any() and not got["projmatrix"][:, 2].any()


@pytest.mark.parametrize("mode", ["dense_cached", "no_cache", "cov3D_precomp", "raw"])
@pytest.mark.parametrize("P", cs.KERNEL_SIZES)
def test_the_kernel_alone(C_, kernel_scenes, P, mode):
    """The operator fed the HIP backward's own sums against the float64 reference fed the same arrays: under one wave (37), one
    wave (64), several workgroups and a ragged last wave (3001), with the forward's SH direction derivatives, without them,
    with a precomputed covariance and from raw parameters.  Measured distances are printed; at 3001 the fp32 chain runs too."""
    s = kernel_scenes[P]
    got, sums, radii = operator_alone(C_, s, mode)
    culled = float((radii == 0).float().mean())
    assert 0.2 <= culled <= 0.5, culled
    ref = reference_of(s, sums, radii, raw=mode == "raw")
    held(got, ref, f"kernel P={P} {mode}")
    if P == 3001 and mode == "dense_cached":
        was = C_.set_f64_chain(False)
        try:
            held(operator_alone(C_, s, mode)[0], ref, f"kernel P={P} fp32 chain")
        finally:
            C_.set_f64_chain(was)


def autograd_reference(s):
    g, cam = s.g, s.cam
    V, F, cp = (T(x).requires_grad_() for x in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))
    col, _, _ = tr.render(T(g["means3D"]), T(g["opacity"]), T(g["scales"]), T(g["rotations"]), T(g["sh"]), torch.tensor(g["degrees"]),
                          V, F, cp, T(cs.BG), s.W, s.H, f32(cam.tanfovx), f32(cam.tanfovy), tiled=True)
    (col * T(s.dl_np)).sum().backward()
    return dict(viewmatrix=V.grad.numpy(), projmatrix=F.grad.numpy(), campos=cp.grad.numpy())


def through_rasterizer(s, needs=(True, True, True), model_grad=False):
    import diff_gaussian_rasterization as dgr
    cams = [t.clone().requires_grad_(n) for t, n in zip((s.vm, s.pm, s.cp), needs)]
    d = s.d
    m3 = d["means3D"].clone().requires_grad_(model_grad)
    m2 = torch.zeros_like(m3, requires_grad=model_grad)
    leaves = [m3, m2] + [d[k].clone().requires_grad_(model_grad) for k in ("opacity", "sh", "scales", "rotations")]
    img, radii = dgr.GaussianRasterizer(s.settings(dgr, *cams))(means3D=m3, means2D=m2, opacities=leaves[2], shs=leaves[3],
                                                                degrees=d["degrees"], scales=leaves[4], rotations=leaves[5])
    return img, radii, cams, leaves


@pytest.mark.parametrize("which", ["kernel 3001", "portrait"])
def test_end_to_end_against_fp64_autograd(C_, kernel_scenes, which):
    """Through GaussianRasterizer with the three camera tensors requiring grad, against fp64 autograd of
    torch_ref.render(tiled=True).  On the code before this feature the three .grad stay None."""
    s = kernel_scenes[3001] if which == "kernel 3001" else Scene(*cs.portrait_scene())
    img, _, cams, _ = through_rasterizer(s)
    assert type(img.grad_fn).__name__ == "_RasterizeGaussiansCamBackward"
    (img * s.dl).sum().backward()
    for name, t in zip(NAMES, cams):
        assert t.grad is not None, f"{name}.grad is None: the camera is not differentiated"
    assert cs.STATE_ROUNDING <= REL / 4   # else the bar would be four times the measured state rounding
    held(dict(zip(NAMES, (t.grad for t in cams))), autograd_reference(s), f"end to end {which}")


def test_gauge_identity_at_20k():
    """Shifting the scene and the camera together changes nothing: sum_i dL_dmeans3D_i = V[:3,:] gV[3,:] + F[:3,:] gF[3,:] -
    g_campos, with the product's own dL_dmeans3D on the left, at 20k Gaussians / 400x400."""
    s = Scene(*cs.gauge_scene())
    img, _, cams, leaves = through_rasterizer(s, model_grad=True)
    (img * s.dl).sum().backward()
    V, F = s.cam.world_view_transform.astype(np.float64), s.cam.full_proj_transform.astype(np.float64)
    gV, gF, gc = (t.grad.cpu().numpy().astype(np.float64) for t in cams)
    lhs = leaves[0].grad.double().sum(0).cpu().numpy()
    rhs = V[:3, :] @ gV[3, :] + F[:3, :] @ gF[3, :] - gc
    res = np.abs(lhs - rhs).max() / np.abs(lhs).max()
    print(f"[camera grad gauge] lhs {lhs}, rhs {rhs}, residual {res:.2e} (tolerance {GAUGE_TOLERANCE:.1e})")
    assert np.abs(lhs).max() > 0 and res <= GAUGE_TOLERANCE


class Model:
    """The reference's GaussianModel, as far as render() looks at it."""

    def __init__(self, s):
        d = s.d
        self._xyz = d["means3D"].clone().requires_grad_(True)
        self._features_dc, self._features_rest = s.dc.clone().requires_grad_(True), s.rest.clone().requires_grad_(True)
        self._opacity = d["opacity"].clone().requires_grad_(True)
        self._scaling, self._rotation = s.raw_scaling.clone().requires_grad_(True), s.raw_rotation.clone().requires_grad_(True)
        self._degrees, self.active_sh_degree, self.max_sh_degree = d["degrees"], 3, 3

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def view_of(s, grad):
    return NS(image_height=s.H, image_width=s.W, FoVx=s.cam.FoVx, FoVy=s.cam.FoVy,
              world_view_transform=s.vm.clone().requires_grad_(grad), full_proj_transform=s.pm.clone().requires_grad_(grad),
              camera_center=s.cp.clone().requires_grad_(grad))


@pytest.mark.parametrize("route", ["raw", "activated"])
def test_nothing_else_moved(C_, kernel_scenes, route):
    """With camera gradients on, the image, the radii and every model gradient equal the existing functions' bit for bit, through
    render() on the raw-parameter route and on the route through GaussianRasterizer; with no camera tensor requiring grad the
    existing autograd functions are the ones that ran."""
    import r3dgs_render
    s = kernel_scenes[3001]
    pipe = NS(debug=False, compute_cov3D_python=route == "activated", convert_SHs_python=False)
    results = {}
    for grad in (False, True):
        pc = Model(s)
        if route == "activated":
            pc.get_covariance = lambda mod, pc=pc: torch.from_numpy(s.cov3D).cuda() + 0.0 * pc._scaling.sum()
        view = view_of(s, grad)
        out = r3dgs_render.render(view, pc, pipe, s.bg)
        name = type(out["render"].grad_fn).__name__
        assert name == {("raw", False): "_RasterizeGaussianParamsBackward", ("raw", True): "_RasterizeGaussianParamsCamBackward",
                        ("activated", False): "_RasterizeGaussiansBackward", ("activated", True): "_RasterizeGaussiansCamBackward"}[
                            (route, grad)], name
        (out["render"] * s.dl).sum().backward()
        results[grad] = [out["render"].detach(), out["radii"], out["viewspace_points"].grad] + \
                        [t.grad for t in pc.leaves() if t.grad is not None]
        cam_grads = [view.world_view_transform.grad, view.full_proj_transform.grad, view.camera_center.grad]
        assert all((t is not None) == grad for t in cam_grads)
        if grad:
            assert all(float(t.abs().max()) > 0 for t in cam_grads)
    assert len(results[False]) == len(results[True]) >= 6
    for k, (a, b) in enumerate(zip(results[False], results[True])):
        assert torch.equal(a, b), (route, k)


def test_determinism_and_a_captured_launch(C_, kernel_scenes):
    """Two runs are bit-identical, end to end and for the operator alone; the operator's call, captured in a torch.cuda.graph on
    the default queue configuration, replays to the eager result bit for bit and follows the buffers it reads."""
    s = kernel_scenes[3001]
    runs = []
    for _ in range(2):
        img, _, cams, _ = through_rasterizer(s)
        (img * s.dl).sum().backward()
        runs.append([t.grad.clone() for t in cams])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    got, sums, radii = operator_alone(C_, s, "dense_cached")
    d, cam = s.d, s.cam
    fout = C_._forward_common(None, s.bg, d["means3D"], EMPTY, d["opacity"], d["scales"], d["rotations"], 1.0, EMPTY, s.vm, s.pm,
                              cam.tanfovx, cam.tanfovy, s.H, s.W, d["sh"], d["degrees"], s.cp, False, False, exact=True)
    fixed = [t.clone() for t in sums]

    def go():
        return C_.camera_backward(d["means3D"], d["degrees"], d["sh"], None, d["scales"], d["rotations"], 1.0, None, False, s.vm, s.pm,
                                  s.cp, cam.tanfovx, cam.tanfovy, s.H, s.W, fout[2], fout[3], *fixed)
    eager = {k: v.clone() for k, v in go().items()}   # warm-up outside the capture (the workspace size is asked here)
    for k in NAMES:
        assert torch.equal(eager[k], got[k]), k
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = go()
    graph.replay()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(static[k], eager[k]), k
    for t in fixed:
        t.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    direct = go()
    for k in NAMES:
        assert torch.equal(static[k], direct[k]) and not torch.equal(static[k], eager[k]), k


def test_edge_cases(C_, kernel_scenes):
    """P == 0 and an all-culled scene give zero tensors; only campos requiring grad produces only that output; a
    QuantisedModel with a camera that requires grad is refused with its message."""
    import diff_gaussian_rasterization as dgr
    import r3dgs_render
    s = kernel_scenes[64]
    z = lambda *shape, **kw: torch.zeros(*shape, device="cuda", **kw)   # noqa: E731
    got = C_.camera_backward(z(0, 3), z(0, 1, dtype=torch.int32), z(0, 16, 3), None, z(0, 3), z(0, 4), 1.0, None, False, s.vm, s.pm,
                             s.cp, 1.0, 1.0, s.H, s.W, z(0, dtype=torch.int32), EMPTY, z(0, 3), z(0, 2, 2), z(0, 3))
    assert all(not got[k].any() for k in NAMES) and got["viewmatrix"].shape == (4, 4) and got["campos"].shape == (3,)
    # an empty model through the autograd function
    cams = [t.clone().requires_grad_(True) for t in (s.vm, s.pm, s.cp)]
    img, _ = dgr.GaussianRasterizer(s.settings(dgr, *cams))(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 16, 3),
                                                            degrees=z(0, 1, dtype=torch.int32), scales=z(0, 3), rotations=z(0, 4))
    img.sum().backward()
    assert all(t.grad is not None and not t.grad.any() for t in cams)
    # everything behind the camera: the kernel reads radii only and the finish writes zeros over whatever was there
    m = s.g["means3D"].copy()
    m[:, 2] = -np.abs(m[:, 2]) - 1.0   # behind the (nearly identity) camera: all culled
    behind = Scene(s.cam, dict(s.g, means3D=m), seed=6)
    got, _, radii = operator_alone(C_, behind, "dense_cached")
    assert not radii.any() and all(not got[k].any() for k in NAMES)
    # only campos
    img, _, cams, _ = through_rasterizer(s, needs=(False, False, True))
    assert type(img.grad_fn).__name__ == "_RasterizeGaussiansCamBackward"
    (img * s.dl).sum().backward()
    assert cams[0].grad is None and cams[1].grad is None and float(cams[2].grad.abs().max()) > 0
    full = through_rasterizer(s)
    (full[0] * s.dl).sum().backward()
    assert torch.equal(cams[2].grad, full[2][2].grad)
    only = C_.camera_backward(s.d["means3D"], s.d["degrees"], None, None, s.d["scales"], s.d["rotations"], 1.0, None, False, s.vm, s.pm,
                              s.cp, s.cam.tanfovx, s.cam.tanfovy, s.H, s.W, *_state_and_sums(C_, s), want=("campos",))
    assert list(only) == ["campos"] and not only["campos"].any()   # (sh = None: precomputed colours, exactly zero)
    # a quantised model
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.__new__(QuantisedModel)
    with pytest.raises(ValueError, match="camera gradients are not available for a QuantisedModel"):
        r3dgs_render.render(view_of(s, True), qm, NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False), s.bg)


def _state_and_sums(C_, s):
    """radii, geomBuffer and the three per-Gaussian sums of a forward + backward over scene `s`."""
    d, cam = s.d, s.cam
    R, _, radii, geom, binning, img = C_._forward_common(
        None, s.bg, d["means3D"], EMPTY, d["opacity"], d["scales"], d["rotations"], 1.0, EMPTY, s.vm, s.pm, cam.tanfovx, cam.tanfovy,
        s.H, s.W, d["sh"], d["degrees"], s.cp, False, False, exact=True)
    back = C_.rasterize_gaussians_backward(s.bg, d["means3D"], radii, EMPTY, d["scales"], d["rotations"], 1.0, EMPTY, s.vm, s.pm,
                                           cam.tanfovx, cam.tanfovy, s.dl, d["sh"], d["degrees"], s.cp, geom, R, binning, img, 0.0,
                                           False, _want_conic=True)
    return radii, geom, back[0], back[8], back[1]


def test_pose_recovery():
    """~400 Gaussians at 64x48, the target rendered at the true pose, the camera started a few hundredths of a radian and of a
    scene unit off, 40 Adam steps on RefinedCamera.xi through render().  The same loop in fp64 through torch_ref reaches
    cs.POSE_RATIO_FP64 (tests/test_camera_grad_cpu.py); the fp32 and fp64 trajectories differ, so the GPU run must reach within a
    factor of two of it, and the pose error must end below where it started."""
    import r3dgs_render
    from r3dgs_camera import RefinedCamera
    cam, g, true, start = cs.pose_target_and_start()
    s = Scene(cam, g)
    pc = Model(s)
    for t in pc.leaves():
        t.requires_grad_(False)
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    with torch.no_grad():
        target = r3dgs_render.render(view_of(s, False), pc, pipe, s.bg)["render"]
    begin = NS(image_height=s.H, image_width=s.W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=start.astype(np.float32),
               projection_matrix=cam.projection_matrix)
    rc = RefinedCamera(begin, device="cuda")
    opt = torch.optim.Adam([rc.xi], lr=cs.POSE_LR)
    err0 = rc.pose_error(true)
    losses = []
    for _ in range(cs.POSE_STEPS + 1):
        loss = (r3dgs_render.render(rc, pc, pipe, s.bg)["render"] - target).abs().mean()
        losses.append(loss)
        if len(losses) > cs.POSE_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    losses = [float(v.detach()) for v in losses]
    ratio, err1 = losses[-1] / losses[0], rc.pose_error(true)
    print(f"[camera grad pose] loss {losses[0]:.4e} -> {losses[-1]:.4e}, ratio {ratio:.3f} (fp64: {cs.POSE_RATIO_FP64:.3f}); "
          f"pose error {err0} -> {err1}")
    assert ratio <= 2 * cs.POSE_RATIO_FP64
    assert err1[0] < err0[0] and err1[1] < err0[1]


def test_refined_camera_builds_its_pose_without_a_host_wait():
    """The three tensors of a RefinedCamera, its snapshot and their backward into xi, evaluated with torch's synchronisation
    debug mode set to 'error': any device-to-host wait raises.  At xi = 0 (the series branch) and at a rotation past the switch."""
    from r3dgs_camera import RefinedCamera
    cam, _ = cs.pose_scene()
    rc = RefinedCamera(cam, device="cuda")
    big = torch.tensor([0.3, -0.2, 0.25, 0.1, 0.2, -0.1], device="cuda")
    weights = [torch.randn(4, 4, device="cuda"), torch.randn(4, 4, device="cuda"), torch.randn(3, device="cuda")]
    torch.cuda.synchronize()
    grads = []
    was = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in range(2):
            rc.xi.grad = None
            parts = [rc.world_view_transform, rc.full_proj_transform, rc.camera_center]
            snap = rc.snapshot()
            parts += [snap.world_view_transform, snap.full_proj_transform, snap.camera_center]
            sum((p * w).sum() for p, w in zip(parts, weights + weights)).backward()
            grads.append(rc.xi.grad.clone())
            with torch.no_grad():
                rc.xi.copy_(big)
    finally:
        torch.cuda.set_sync_debug_mode(was)
    for g in grads:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    want = torch.linalg.matrix_exp(torch.tensor([[0, -0.25, -0.2, 0.1], [0.25, 0, -0.3, 0.2], [0.2, 0.3, 0, -0.1], [0, 0, 0, 0]],
                                                dtype=torch.float64))
    got = (torch.linalg.inv(rc.W0.double().cpu()) @ rc.world_view_transform.detach().double().cpu()).t()
    assert float((got - want).abs().max()) <= 1e-5
