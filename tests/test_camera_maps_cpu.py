"""CPU tests of the maps' share of a camera gradient (include/r3dgs_camera.h r3dgs_camera_backward_maps, camera_math.h
camera_maps_gaussian, render(camera_grad_maps=True)): the float64 reference tests/camera_maps_ref.py pinned to finite
differences, the per-Gaussian function run on the host (tests/hostcheck_camera_maps) against it, its agreement with the colour
route's function at dL_dz = 0, the structural zeros, a hand case, the share of masked pixels of the GPU scenes, and the host
surface with fakes.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import aux_ref as ar
from tests import camera_grad_scenes as cs
from tests import camera_maps_ref as cmr
from tests import camera_maps_scenes as cms
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_MAX_FRACTION = 1e-3


@pytest.fixture(scope="module")
def shim():
    lib = build_shim(os.path.join(HERE, "hostcheck_camera_maps", "hostcheck_camera_maps.hip"),
                     os.path.join(HERE, "hostcheck_camera_maps", "libhostcheck_camera_maps.so"), EXACT, None)
    assert lib.hc_cam_map_sums() == 24
    return lib


def fp(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(C.c_void_p)


def run_shim(lib, cam, g, radii, g2, gcon, gz, f64=True, colour_route=False, shares=False, cov3D=None):
    """-> (dL_dviewmatrix [4,4], dL_dprojmatrix [4,4] as float32, the 24 sums, the 24 sums of absolute shares[, shares])."""
    P = len(g["means3D"])
    keep = [fp(cam.world_view_transform), fp(cam.full_proj_transform), fp(radii, np.int32), fp(g["means3D"]), fp(g["scales"]),
            fp(g["rotations"]), fp(g2), fp(gcon), fp(gz), fp(np.zeros(1) if cov3D is None else cov3D)]
    sums, abs_sums = np.zeros(24), np.zeros(24)
    rows = np.zeros((P, 24)) if shares else None
    lib.hc_camera_maps(P, int(f64), int(colour_route), cam.image_width, cam.image_height, C.c_float(cam.tanfovx), C.c_float(cam.tanfovy),
                       C.c_float(1.0), keep[0][1], keep[1][1], keep[2][1], keep[3][1], keep[4][1], keep[5][1], None if cov3D is None else keep[9][1], keep[6][1],
                       keep[7][1], keep[8][1], sums.ctypes.data_as(C.c_void_p), abs_sums.ctypes.data_as(C.c_void_p),
                       None if rows is None else rows.ctypes.data_as(C.c_void_p))
    gv, gf = np.zeros(16, np.float32), np.zeros(16, np.float32)
    lib.hc_camera_maps_entries(sums.ctypes.data_as(C.c_void_p), gv.ctypes.data_as(C.c_void_p), gf.ctypes.data_as(C.c_void_p))
    out = (gv.reshape(4, 4), gf.reshape(4, 4), sums, abs_sums)
    return out + (rows,) if shares else out


def sums_as_matrices(sums):
    """The 24 double sums in the outputs' layout, without the rounding to fp32."""
    gv, gf = np.zeros((4, 4)), np.zeros((4, 4))
    gv[:, :3] = sums[:12].reshape(4, 3)
    gf[:, [0, 1, 3]] = sums[12:].reshape(4, 3)
    return gv, gf


class Small:
    """A scene small enough for finite differences: the oracle's state, the unmasked pixels, seeded upstream gradients."""

    def __init__(self, P=37):
        self.cam, self.g = cms.kernel_scene(P)
        out = cs.oracle_forward(self.cam, self.g)
        self.st, self.radii = out["state"], out["radii"]
        H, W = self.cam.image_height, self.cam.image_width
        ok = ~((out["ambig"].reshape(-1) != 0) | ar.aux_ref(self.st)["median_ambig"].reshape(-1))
        rng = np.random.default_rng(3)
        gs = [rng.uniform(-1.0, 1.0, H * W) * ok for _ in range(4)]
        self.F = rng.uniform(-1.0, 1.0, (P, 5))
        self.up = dict(depth=gs[0], alpha=gs[1], median_depth=gs[2], distortion=(gs[3], 0.5, 50.0),
                       features=(self.F, rng.uniform(-1.0, 1.0, (5, H * W)) * ok))


@pytest.fixture(scope="module")
def small():
    return Small()


@pytest.fixture(scope="module")
def small_ref(small):
    return cmr.camera_grads(small.st, small.g, small.cam, small.up)


def test_reference_is_pinned_to_finite_differences(small, small_ref):
    """Central differences of the float64 loss in every non-structural entry of V and F, at frozen decisions: 1e-6 of the
    tensor's maximum."""
    s, ref = small, small_ref
    for name, cols in (("viewmatrix", (0, 1, 2)), ("projmatrix", (0, 1, 3))):
        base = (s.cam.world_view_transform if name == "viewmatrix" else s.cam.full_proj_transform).astype(np.float64)
        fd = np.zeros((4, 4))
        for j in range(4):
            for i in cols:
                h = 1e-6 * max(1.0, abs(base[j, i]))
                vals = []
                for sign in (1.0, -1.0):
                    m = base.copy()
                    m[j, i] += sign * h
                    kw = dict(V=m) if name == "viewmatrix" else dict(Fm=m)
                    vals.append(cmr.camera_grads(s.st, s.g, s.cam, s.up, **kw)["loss"])
                fd[j, i] = (vals[0] - vals[1]) / (2 * h)
        scale = np.abs(ref[name]).max()
        err = np.abs(fd - ref[name]).max()
        print(f"[camera maps fd] {name}: max err {err:.3e}, max |ref| {scale:.3e}")
        assert scale > 0 and err <= 1e-6 * scale
        dead = [i for i in range(4) if i not in cols]
        assert not ref[name][:, dead].any()   # column 3 of V, column 2 of F: never read


@pytest.mark.parametrize("P", [37, 3001])
def test_host_function_against_the_reference(shim, P):
    """camera_maps_gaussian fed the reference's own per-Gaussian (xy, conic, z) gradients, against the float64 evaluation of
    the same stage with the conventions r3dgs_camera_backward documents (camera_maps_ref.chained): in double to 1e-10 of each
    tensor's maximum, in fp32 within the project's 1e-4.  Both sides read the same fp32 numbers: the gradients rounded to fp32
    and the oracle's fp32 cov3D.  (The pure autograd chain through aux_grad_ref.geometry has neither the 1e-7 beside det^2 nor
    the fp32 focal lengths: it is held to the whole pass at 1e-4 on the GPU, and to finite differences above.)
    The new dL_dz term of `chained` is one numpy line, gV[:, 2] += sum dL_dz [m, 1], which restates the term under test: at
    1e-10 that term is pinned by the hand case below and, independently of any restatement, by the plain-autograd comparison
    at the end of this test (z = (mt V)_2 differentiated by torch) at 0.25e-4 and by finite differences at 1e-6."""
    s = Small(P) if P != 37 else Small()
    up = dict(depth=s.up["depth"], alpha=s.up["alpha"], median_depth=s.up["median_depth"]) if P == 3001 else s.up
    pg = cmr.camera_grads(s.st, s.g, s.cam, up)
    pg32 = {k: np.asarray(pg[k], np.float32).astype(np.float64) for k in ("means2D", "conic", "z")}
    cov3D = np.asarray(s.st["cov3D"], np.float32).reshape(-1, 6)
    want = cmr.chained(s.g, s.cam, pg32, s.radii, cov3D)
    for f64, bar in ((True, 1e-10), (False, 1e-4)):
        _, _, sums, _ = run_shim(shim, s.cam, s.g, s.radii, pg32["means2D"], pg32["conic"], pg32["z"], f64=f64, cov3D=cov3D)
        for name, got in zip(("viewmatrix", "projmatrix"), sums_as_matrices(sums)):
            scale = np.abs(want[name]).max()
            err = np.abs(got - want[name]).max()
            print(f"[camera maps host P={P} f64={f64}] {name}: max err {err:.3e}, bar {bar * scale:.3e}")
            assert scale > 0 and err <= bar * scale
    # the conventions are worth little: the same stage by plain autograd (the end-to-end reference's own two tensors)
    for name in ("viewmatrix", "projmatrix"):
        err = np.abs(cmr.chained(s.g, s.cam, pg, s.radii, cov3D)[name] - pg[name]).max() / np.abs(pg[name]).max()
        print(f"[camera maps host P={P}] {name}: conventions against plain autograd {err:.3e}")
        assert err <= 0.25e-4


@pytest.mark.parametrize("f64", [True, False])
def test_zero_depth_gradient_is_the_colour_route_bit_for_bit(shim, small, small_ref, f64):
    s, pg = small, small_ref
    zero = np.zeros(len(s.radii))
    a = run_shim(shim, s.cam, s.g, s.radii, pg["means2D"], pg["conic"], zero, f64=f64, shares=True)
    b = run_shim(shim, s.cam, s.g, s.radii, pg["means2D"], pg["conic"], zero, f64=f64, colour_route=True, shares=True)
    assert np.abs(a[2]).max() > 0
    assert a[2].tobytes() == b[2].tobytes() and a[4].tobytes() == b[4].tobytes()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert not a[0][:, 3].any() and not a[1][:, 2].any()   # the structural zeros, exactly


def test_one_gaussian_on_the_optical_axis(shim):
    """Depth loss only: dL_dviewmatrix[4 k + 2] = dL_dz * [m, 1][k] -- entry 14 is dL_dz itself -- and nothing else."""
    cam = ss.Camera(32, 32, 30.0, 30.0)
    m = np.array([[0.25, -0.5, 4.0]], np.float32)
    g = dict(means3D=m, scales=np.full((1, 3), 0.1, np.float32), rotations=np.array([[1.0, 0, 0, 0]], np.float32))
    dz = 0.375
    for f64 in (True, False):
        gv, gf, _, _ = run_shim(shim, cam, g, np.array([3]), np.zeros((1, 2)), np.zeros((1, 3)), np.array([dz]), f64=f64)
        want = np.zeros((4, 4), np.float32)
        want[:, 2] = dz * np.array([0.25, -0.5, 4.0, 1.0])
        assert np.array_equal(gv, want) and gv.reshape(-1)[14] == np.float32(dz) and not gf.any()
    gv, gf, _, _ = run_shim(shim, cam, g, np.array([0]), np.zeros((1, 2)), np.zeros((1, 3)), np.array([dz]))
    assert not gv.any() and not gf.any()   # culled: no share


def test_masked_pixels_of_the_gpu_scenes():
    """The oracle's threshold-ambiguous pixels plus aux_ref's median-near-0.5 pixels: at most 0.1 % of each GPU scene
    (tests/camera_maps_scenes.py: 0 of 6144, 4 of 6144 and 15 of 23751 pixels)."""
    for name, (cam, g) in (("kernel 64", cms.kernel_scene(64)), ("kernel 3001", cms.kernel_scene(3001)),
                           ("portrait", cms.portrait_scene())):
        out = cs.oracle_forward(cam, g)
        masked = (out["ambig"].reshape(-1) != 0) | ar.aux_ref(out["state"])["median_ambig"].reshape(-1)
        print(f"[camera maps masks] {name}: {int(masked.sum())} of {masked.size} pixels, {masked.mean():.5f}")
        assert masked.mean() <= FLAG_MAX_FRACTION, name


def scene_upstreams(cam, st, ambig, P):
    """Seeded upstream gradients of every map of a GPU scene, zero on the masked pixels -> the reference's `up` per configuration."""
    H, W = cam.image_height, cam.image_width
    ok = ~((np.asarray(ambig).reshape(-1) != 0) | ar.aux_ref(st)["median_ambig"].reshape(-1))
    rng = np.random.default_rng(17)
    u = lambda *shape: (rng.uniform(-1.0, 1.0, shape) * ok).astype(np.float32)   # noqa: E731
    F = rng.uniform(-1.0, 1.0, (P, 5)).astype(np.float32)
    d = dict(depth=u(H * W), alpha=u(H * W), median_depth=u(H * W), dist=u(H * W), feat=u(5, H * W))
    return dict(aux={k: d[k] for k in ("depth", "alpha", "median_depth")}, dist_lin=dict(distortion=(d["dist"], 0.0, 0.0)),
                dist_nf=dict(distortion=(d["dist"], 0.5, 50.0)), feat=dict(features=(F, d["feat"])))


def test_state_rounding_of_the_end_to_end_scenes():
    """The tolerance of the end-to-end GPU test: what the fp32 forward state alone is worth -- the reference walking the
    oracle's fp32 state against end-to-end float64, per map and tensor, on the three GPU scenes.  cms.STATE_ROUNDING is the
    worst figure measured here; it stays under a quarter of the gradient bar, so the GPU test keeps the bar."""
    worst = 0.0
    for name, (cam, g) in (("kernel 64", cms.kernel_scene(64)), ("kernel 3001", cms.kernel_scene(3001)),
                           ("portrait", cms.portrait_scene())):
        out = cs.oracle_forward(cam, g)
        for which, up in scene_upstreams(cam, out["state"], out["ambig"], len(g["means3D"])).items():
            want = cmr.camera_grads(out["state"], g, cam, up)
            got = cmr.camera_grads(out["state"], g, cam, up, state_values=True)
            for k in ("viewmatrix", "projmatrix"):
                e = float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max())
                print(f"[camera maps state rounding, {name}, {which}] {k}: {e:.3e}")
                worst = max(worst, e)
    print(f"[camera maps state rounding] worst {worst:.4e}")
    assert abs(worst - cms.STATE_ROUNDING) <= 0.01 * cms.STATE_ROUNDING, worst
    assert cms.STATE_ROUNDING <= 1e-4 / 4   # the end-to-end GPU test keeps the project's bar


def test_pose_recovery_in_fp64():
    """The loop of the GPU pose test in float64 through the reference: POSE_STEPS Adam steps at POSE_LR on xi, a depth + alpha
    loss only (no colour), the decisions of every step frozen by the oracle's fp32 forward at that step's pose.  Its final /
    initial loss ratio, cms.POSE_RATIO_FP64, is what the GPU run is held to."""
    from oracle import oracle as orc
    from r3dgs_camera import RefinedCamera, se3_exp
    from tests import aux_grad_ref as agr
    cam, g, true, start = cs.pose_target_and_start()
    W, H = cam.image_width, cam.image_height
    proj = cmr.T(cam.projection_matrix)
    m3, op, sc, rot = (cmr.T(g[k]) for k in ("means3D", "opacity", "scales", "rotations"))

    def maps(wv):
        Fm = wv @ proj
        f32 = lambda t: t.detach().numpy().astype(np.float32)   # noqa: E731
        out = orc.forward(cs.BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, f32(wv), f32(Fm),
                          cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], f32(RefinedCamera.center_of(wv)))
        got = agr.walk(out["state"], *agr.geometry(m3, op.reshape(-1, 1), sc, rot, wv, Fm, W, H, cam.tanfovx, cam.tanfovy))
        return got["depth"], got["alpha"]
    with torch.no_grad():
        tdepth, talpha = maps(cmr.T(true))
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=cs.POSE_LR)
    losses = []
    for _ in range(cs.POSE_STEPS + 1):
        depth, alpha = maps(cmr.T(start) @ se3_exp(xi).t())
        loss = (depth - tdepth).abs().mean() + (alpha - talpha).abs().mean()
        losses.append(float(loss.detach()))
        if len(losses) > cs.POSE_STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    ratio = losses[-1] / losses[0]
    print(f"[camera maps pose, fp64] loss {losses[0]:.4e} -> {losses[-1]:.4e}, ratio {ratio:.4f}")
    assert abs(ratio - cms.POSE_RATIO_FP64) <= 0.01 * cms.POSE_RATIO_FP64, ratio
    assert ratio < 0.5


def test_host_surface():
    import inspect

    import diff_gaussian_rasterization as dgr
    import r3dgs_camera
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    rows = _C._ABI["required"][1]
    assert len(rows["r3dgs_camera_backward_maps"][1]) == 20 and len(rows["r3dgs_camera_backward_maps_workspace_bytes"][1]) == 1
    for sib, scr in (("r3dgs_aux_maps_backward", "r3dgs_aux_maps_backward_screen"),
                     ("r3dgs_distortion_map_backward", "r3dgs_distortion_backward_screen"),
                     ("r3dgs_feature_maps_backward", "r3dgs_feature_maps_backward_screen")):
        assert rows[scr][1][:-4] == rows[sib][1][:-2] and rows[scr][1][-4:] == [C.c_void_p] * 4
    assert _C._lib.r3dgs_camera_backward_maps_workspace_bytes(0) == 0
    assert _C._lib.r3dgs_camera_backward_maps_workspace_bytes(3001) >= 12 * 24 * 8
    assert _C._lib.r3dgs_camera_backward_maps_workspace_bytes(10 ** 9) == _C._lib.r3dgs_camera_backward_maps_workspace_bytes(10 ** 8)
    assert _C.CAMERA_MAP_GRADS == ("viewmatrix", "projmatrix") and _C.SCREEN_GRADS == ("conic", "z")
    for cls, base in ((dgr._AuxMapsCam, dgr._AuxMaps), (dgr._DistortionMapCam, dgr._DistortionMap), (dgr._FeatureMapsCam, dgr._FeatureMaps)):
        assert issubclass(cls, torch.autograd.Function)
        assert list(inspect.signature(cls.forward).parameters)[:-2] == list(inspect.signature(base.forward).parameters)
        assert list(inspect.signature(cls.forward).parameters)[-2:] == ["viewmatrix", "projmatrix"]
    z = torch.zeros
    args = dict(means3D=z(4, 3), scales=z(4, 3), rotations=z(4, 4), scale_modifier=1.0, cov3D_precomp=None, viewmatrix=torch.eye(4),
                projmatrix=torch.eye(4), tanfovx=1.0, tanfovy=1.0, image_height=16, image_width=16, radii=z(4, dtype=torch.int32),
                dL_dmeans2D=z(4, 3), dL_dconic=z(4, 4), dL_dz=z(4))
    with pytest.raises(RuntimeError, match="camera_backward_maps: means3D: .*no CPU path"):
        _C.camera_backward_maps(**args)
    with pytest.raises(ValueError, match="unknown gradient"):
        _C.camera_backward_maps(**args, want=("campos",))
    with pytest.raises(ValueError, match="unknown gradient"):   # the screen-space names belong to the _screen forms alone
        _C.aux_maps_backward(0, 0, 16, 16, z(0), z(0), z(0), None, None, 1.0, 1.0, z(0, 3), None, 1.0, None, None, None, want=("conic",))
    # render(): keyword off -- the three refusals stand, before anything is launched; on -- they do not, the others do
    cam = r3dgs_camera.RefinedCamera(ss.Camera(32, 32, 30.0, 30.0), device="cpu")
    for kw, msg in ((dict(aux=("depth",), aux_grad=True), "aux_grad=True together with a camera that requires grad"),
                    (dict(distortion=True), "distortion together with a camera that requires grad")):
        with pytest.raises(ValueError, match=msg):
            r3dgs_render.render(cam, _Model(), None, None, **kw)
        with pytest.raises(_Launched):
            r3dgs_render.render(cam, _Model(), _Pipe(True), None, camera_grad_maps=True, **kw)
    # (features must live on a device before their geometry refusal is reached: that one is asked directly)
    with pytest.raises(ValueError, match="features_geom_grad=True together with a camera that requires grad"):
        r3dgs_render._checked_geom_grad(_Model(), cam)
    r3dgs_render._checked_geom_grad(_Model(), cam, True)
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.__new__(QuantisedModel)
    with pytest.raises(ValueError, match="camera gradients are not available for a QuantisedModel"):
        r3dgs_render.render(cam, qm, None, None, aux=("depth",), aux_grad=True, camera_grad_maps=True)
    with pytest.raises(ValueError, match="normals=True together with a camera that requires grad"):
        r3dgs_render.render(cam, _Model(), _Pipe(False), None, normals=True, camera_grad_maps=True)
    with pytest.raises(ValueError, match="antialiasing=True together with a camera that requires grad"):
        r3dgs_render.render(cam, _Model(), _Pipe(False), None, antialiasing=True, camera_grad_maps=True)
    with torch.no_grad():   # a camera that does not require grad: the keyword is a no-op, aux_grad's own refusal speaks
        with pytest.raises(ValueError, match="aux_grad=True under no_grad"):
            r3dgs_render.render(cam, _Model(), _Pipe(True), None, aux=("depth",), aux_grad=True, camera_grad_maps=True)


class _Launched(Exception):
    """Raised by the fake model where render() would start to read the model for the forward: past every refusal."""


class _Pipe:
    debug = False
    convert_SHs_python = False

    def __init__(self, launches):
        self.launches = launches

    @property
    def compute_cov3D_python(self):
        if self.launches:
            raise _Launched()
        return False


class _Model:
    """A model on the host with four Gaussians: enough for the checks in front of the forward."""
    active_sh_degree = max_sh_degree = 0

    def __init__(self):
        self._xyz = torch.zeros(4, 3)
        self._scaling = torch.zeros(4, 3)
        self._rotation = torch.zeros(4, 4)
        self._opacity = torch.zeros(4, 1)
