"""GPU tests (-m gpu) of the raw-parameter path: r3dgs_forward_params* / r3dgs_backward_params / r3dgs_activate_params,
diff_gaussian_rasterization.rasterize_gaussian_params and r3dgs_render.render.

The fused path is checked against the EXISTING path fed what the fused kernels compute internally -- the activated values
r3dgs_activate_params returns (the same param_math.h functions) and torch.cat of the two SH tensors: image, radii,
num_rendered and the exported binning bit for bit; dL_dmeans3D / dL_dmeans2D / dL_dopacity and the two SH gradients (as
slices of the joined one, zeros included, into NaN-filled buffers) bit for bit; dL_dscaling / dL_drotation bit for bit
against the host shim's restatement of param_math.h's backward applied to the existing path's dL_dscale / dL_drot."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth_scene as ss
from tests import test_params_cpu as host

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_scenes = {}


def scene(name):
    """-> dict of device tensors shaped as GaussianModel stores them (raw), plus camera / image size."""
    if name in _scenes:
        return _scenes[name]
    if name.startswith("small"):
        W, H, P = 400, 304, 20_000 + 37   # P not a multiple of 64: the tail wave's scalar path
        cam = ss.make_camera(W, H, 300.0, 3)
        g = ss.make_gaussians(P, cam, seed=11, degree_mode="mixed" if name == "small_mixed" else "all3", scale_mu=0.03)
    else:
        w, cam, g = ss.make_workload({"metric": "metric_500k_1600x1062", "clustered": "clustered_500k_1600x1062"}[name], seed=0)
        W, H, P = w["W"], w["H"], w["P"]
        if name == "clustered":   # mixed degrees on the clustered scene (the metric scene stays all-degree-3)
            g["degrees"] = (np.arange(P) % 4).astype(np.int32)
    rng = np.random.default_rng(5)
    rot_raw = (g["rotations"] * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)   # unnormalised, as a trained model's
    s = dict(W=W, H=H, P=P, cam=cam, xyz=_dev(g["means3D"]), dc=_dev(g["sh"][:, :1]), rest=_dev(g["sh"][:, 1:]),
             opacity=_dev(g["opacity"]), scaling=_dev(np.log(g["scales"]).astype(np.float32)), rotation=_dev(rot_raw),
             degrees=_dev(g["degrees"]), bg=_dev(np.array([0.1, 0.2, 0.3], np.float32)), vm=_dev(cam.world_view_transform),
             pm=_dev(cam.full_proj_transform), cp=_dev(cam.camera_center), dL=_dev(ss.upstream_grad(W, H, seed=1) * (W * H)))
    if len(_scenes) >= 2:   # two 500 k scenes at most stay resident
        _scenes.pop(next(iter(_scenes)))
    _scenes[name] = s
    return s


def fused_forward(_C, s, exact, reserve):
    c = s["cam"]
    return _C.rasterize_gaussian_params(s["bg"], s["xyz"], s["dc"], s["rest"], s["degrees"], s["opacity"], s["scaling"],
                                        s["rotation"], 1.0, s["vm"], s["pm"], c.tanfovx, c.tanfovy, s["H"], s["W"], s["cp"],
                                        False, False, exact=exact, _reserve=reserve)


def existing_forward(_C, s, act, sh, exact, reserve):
    c = s["cam"]
    return _C._forward_common(None, s["bg"], s["xyz"], EMPTY, s["opacity"], act[0], act[1], 1.0, EMPTY, s["vm"], s["pm"],
                              c.tanfovx, c.tanfovy, s["H"], s["W"], sh, s["degrees"], s["cp"], False, False, exact=exact,
                              _reserve=reserve)


def fused_backward(_C, s, out, lam):
    c = s["cam"]
    nr, _, radii, geom, binning, img = out
    return _C.rasterize_gaussian_params_backward(s["bg"], s["xyz"], radii, s["dc"], s["rest"], s["degrees"], s["opacity"],
                                                 s["scaling"], s["rotation"], 1.0, s["vm"], s["pm"], c.tanfovx, c.tanfovy,
                                                 s["dL"], s["cp"], geom, nr, binning, img, lam, False)


def fused_backward_into_nan(_C, s, out, lam):
    """The C entry point itself, every output pre-filled with NaN: each element must have been written."""
    c = s["cam"]
    nr, _, radii, geom, binning, img = out
    P, M = s["P"], 1 + s["rest"].shape[1]
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    o = dict(m2d=nan(P, 3), op=nan(P, 1), col=nan(P, 3), m3d=nan(P, 3), cov=nan(P, 6), dc=nan(P, 1, 3), rest=nan(P, M - 1, 3),
             sc=nan(P, 3), rot=nan(P, 4))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = _C._lib.r3dgs_backward_params(P, p(s["degrees"]), M, int(nr.capacity), p(s["bg"]), s["W"], s["H"], p(s["xyz"]), p(s["dc"]),
                                       p(s["rest"]), p(s["scaling"]), 1.0, p(s["rotation"]), p(s["vm"]), p(s["pm"]), p(s["cp"]),
                                       c.tanfovx, c.tanfovy, p(radii), p(geom), p(binning) if binning.numel() else None, p(img),
                                       p(s["dL"]), p(o["m2d"]), None, p(o["op"]), p(o["col"]), p(o["m3d"]), p(o["cov"]), p(o["dc"]),
                                       p(o["rest"]), p(o["sc"]), p(o["rot"]), lam, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, _C._lib.r3dgs_last_error()
    torch.cuda.synchronize()
    return o


def existing_backward(_C, s, act, sh, out, lam):
    c = s["cam"]
    nr, _, radii, geom, binning, img = out
    return _C.rasterize_gaussians_backward(s["bg"], s["xyz"], radii, EMPTY, act[0], act[1], 1.0, EMPTY, s["vm"], s["pm"],
                                           c.tanfovx, c.tanfovy, s["dL"], sh, s["degrees"], s["cp"], geom, nr, binning, img, lam,
                                           False)


def host_activation_backward(s, act, dL_dscale, dL_drot):
    """param_math.h's backward on the host (tests/hostcheck_params): IEEE operations only, so the kernels must agree
    bit for bit.  The norm comes from the host's quat_act on the same raw quaternions."""
    lib = host.shim()
    q_host, n = host.host_quat_act(lib, s["rotation"].cpu().numpy())
    q_dev = act[1].cpu().numpy()
    assert np.array_equal(q_host.view(np.uint32), q_dev.view(np.uint32)), "normalize: host and device disagree"
    want_rot = host.host_quat_act_bwd(lib, q_dev, n, dL_drot.cpu().numpy())
    want_sc = host.host_scale_act_bwd(lib, dL_dscale.cpu().numpy().reshape(-1), act[0].cpu().numpy().reshape(-1)).reshape(-1, 3)
    return want_sc, want_rot


def bits_equal(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


CASES = [(sc, lam, path, chain, binding)
         for sc in ("small_mixed", "small_all3", "metric", "clustered")
         for lam in (0.0, 0.1) for path in ("reserved", "exact") for chain in (True, False) for binding in ("torch", "ctypes")]


@pytest.mark.parametrize("scene_name,lam,path,chain,binding", CASES)
def test_fused_equals_existing_path(scene_name, lam, path, chain, binding):
    from diff_gaussian_rasterization import _C
    s = scene(scene_name)
    was_binding, was_chain = _C.set_binding(binding), _C.set_f64_chain(chain)
    try:
        act = _C.activate_params(s["scaling"], s["rotation"])
        sh = torch.cat((s["dc"], s["rest"]), dim=1)
        exact = path == "exact"
        reserve = None
        if not exact:   # one reservation for both sides, from the pair count of an exact pass, with room to spare
            pairs = existing_forward(_C, s, act, sh, True, None)[0].pairs
            reserve = int(pairs * 1.25) + 4096
        out_e = existing_forward(_C, s, act, sh, exact, reserve)
        out_f = fused_forward(_C, s, exact, reserve)
        # ---- forward, bit for bit
        assert int(out_f[0]) == int(out_e[0]) and out_f[0].pairs == out_e[0].pairs
        assert not out_f[0].truncated and not out_e[0].truncated
        assert torch.equal(out_f[1], out_e[1]), "image"
        assert torch.equal(out_f[2], out_e[2]), "radii"
        ex_e = _C.export_binning(s["P"], out_e[0], s["H"], s["W"], out_e[3], out_e[4], out_e[5])
        ex_f = _C.export_binning(s["P"], out_f[0], s["H"], s["W"], out_f[3], out_f[4], out_f[5])
        for k in ex_e:
            assert torch.equal(ex_e[k], ex_f[k]), k
        # ---- backward
        ge = existing_backward(_C, s, act, sh, out_e, lam)   # m2d, colors, opacity, m3d, cov3D, sh, scales, rotations
        gf = fused_backward(_C, s, out_f, lam)               # m2d, opacity, xyz, dc, rest, scaling, rotation
        gn = fused_backward_into_nan(_C, s, out_f, lam)
        assert bits_equal(gf[0], ge[0]) and bits_equal(gf[1], ge[2]) and bits_equal(gf[2], ge[3])
        assert bits_equal(gf[3], ge[5][:, :1].contiguous()), "dL_dfeatures_dc"
        assert bits_equal(gf[4], ge[5][:, 1:].contiguous()), "dL_dfeatures_rest"
        want_sc, want_rot = host_activation_backward(s, act, ge[6], ge[7])
        assert bits_equal(gf[5], want_sc), "dL_dscaling_raw"
        assert bits_equal(gf[6], want_rot), "dL_drotation_raw"
        # the C entry point wrote every element of NaN-filled buffers, the zeros above the degree and of culled rows included
        for k, ref in (("m2d", gf[0]), ("op", gf[1]), ("m3d", gf[2]), ("dc", gf[3]), ("rest", gf[4]), ("sc", gf[5]), ("rot", gf[6]),
                       ("col", ge[1]), ("cov", ge[4])):
            assert not torch.isnan(gn[k]).any(), k
            assert bits_equal(gn[k], ref), k
        culled = out_f[2] == 0
        assert culled.any() and (gf[4][culled] == 0).all() and (gf[3][culled] == 0).all()
        deg = s["degrees"].long().reshape(-1)
        above = torch.arange(1, 16, device="cuda")[None, :] >= ((deg + 1) ** 2)[:, None]
        assert (gf[4][above] == 0).all()
        assert gf[4].abs().max() > 0 and gf[5].abs().max() > 0 and gf[6].abs().max() > 0
    finally:
        _C.set_binding(was_binding)
        _C.set_f64_chain(was_chain)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_strict_redo_and_lossy_opt_out(binding):
    """tests/test_train_loop_gpu.py's test of that name for the raw-parameter forward, at its shape: the same overflowing
    reservation through strict mode (default: result == exact path, one redo counted) and with strict mode off (farthest
    pairs dropped, pass flagged)."""
    from diff_gaussian_rasterization import _C
    W, H, P = 320, 240, 8000
    cam = ss.make_camera(W, H, 250.0, 6)
    g = ss.make_gaussians(P, cam, seed=41, degree_mode="all3", scale_mu=0.03)
    args = (_dev(np.array([0.3, 0.2, 0.1], np.float32)), _dev(g["means3D"]), _dev(g["sh"][:, :1]), _dev(g["sh"][:, 1:]),
            _dev(g["degrees"]), _dev(g["opacity"]), _dev(np.log(g["scales"]).astype(np.float32)), _dev(g["rotations"]), 1.0,
            _dev(cam.world_view_transform), _dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, H, W,
            _dev(cam.camera_center), False, False)
    was = _C.set_binding(binding)
    try:
        exact = _C.rasterize_gaussian_params(*args, exact=True)
        R = exact[0].pairs
        s0 = _C.pass_stats()
        out = _C.rasterize_gaussian_params(*args, _reserve=R // 2)            # strict (default)
        s1 = _C.pass_stats()
        assert s1["redone_passes"] == s0["redone_passes"] + 1
        assert not out[0].truncated and out[0].pairs == R and int(out[0]) == int(exact[0])
        assert torch.equal(out[1], exact[1]) and torch.equal(out[2], exact[2])
        lossy = _C.rasterize_gaussian_params(*args, _reserve=R // 2, _strict_override=False)
        assert lossy[0].truncated and not torch.equal(lossy[1], exact[1])
    finally:
        _C.set_binding(was)


def test_odd_coefficient_counts_and_dc_only():
    """M = 1 (no features_rest), M = 4 and M = 9: the scalar / general staging paths."""
    from diff_gaussian_rasterization import _C
    s0 = scene("small_mixed")
    for M in (1, 4, 9):
        s = dict(s0)
        s["rest"] = s0["rest"][:, :M - 1].contiguous()
        s["degrees"] = torch.clamp(s0["degrees"], max=int(math.isqrt(M)) - 1)
        act = _C.activate_params(s["scaling"], s["rotation"])
        sh = torch.cat((s["dc"], s["rest"]), dim=1)
        for lam in (0.0, 0.1):
            out_e = existing_forward(_C, s, act, sh, True, None)
            out_f = fused_forward(_C, s, True, None)
            assert torch.equal(out_f[1], out_e[1]) and torch.equal(out_f[2], out_e[2])
            ge, gf = existing_backward(_C, s, act, sh, out_e, lam), fused_backward(_C, s, out_f, lam)
            assert bits_equal(gf[3], ge[5][:, :1].contiguous()) and bits_equal(gf[2], ge[3])
            if M > 1:
                assert bits_equal(gf[4], ge[5][:, 1:].contiguous())
            else:
                assert gf[4].shape == (s["P"], 0, 3)


def test_activate_against_torch():
    """r3dgs_activate_params against exp / F.normalize in float64; bar: twice what torch's own fp32 operators reach on the
    same device and inputs."""
    from diff_gaussian_rasterization import _C
    gen = torch.Generator(device="cuda").manual_seed(3)
    n = 1 << 20
    scaling = (torch.rand(n, 3, device="cuda", generator=gen) * 40 - 20).contiguous()
    rotation = torch.randn(n, 4, device="cuda", generator=gen) * torch.pow(10.0, torch.rand(n, 1, device="cuda", generator=gen) * 6 - 3)
    rotation = rotation.contiguous()
    s, q = _C.activate_params(scaling, rotation)
    ref_s, ref_q = torch.exp(scaling.double()), F.normalize(rotation.double(), dim=1)
    rel = lambda x: ((x.double() - ref_s).abs() / ref_s).max().item()
    ours_s, torch_s = rel(s), rel(torch.exp(scaling))
    ours_q = (q.double() - ref_q).abs().max().item()
    torch_q = (F.normalize(rotation, dim=1).double() - ref_q).abs().max().item()
    print(f"\nactivate vs float64: exp max rel err ours {ours_s:.3e} torch fp32 {torch_s:.3e}; "
          f"normalize max abs err ours {ours_q:.3e} torch fp32 {torch_q:.3e}")
    assert ours_s <= 2 * torch_s
    assert ours_q <= 2 * torch_q
    for binding in ("torch", "ctypes"):
        was = _C.set_binding(binding)
        try:
            s2, q2 = _C.activate_params(scaling, rotation)
        finally:
            _C.set_binding(was)
        assert torch.equal(s2, s) and torch.equal(q2, q)


# ---- end to end through r3dgs_render.render ----------------------------------------------------------------------------

class Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


class Cam:
    def __init__(self, s):
        c = s["cam"]
        self.FoVx, self.FoVy = 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy)
        self.image_height, self.image_width = s["H"], s["W"]
        self.world_view_transform, self.full_proj_transform, self.camera_center = s["vm"], s["pm"], s["cp"]


class Model:
    """GaussianModel-shaped stand-in: the raw leaves and the activations the reference's properties apply."""
    max_sh_degree = active_sh_degree = 3

    def __init__(self, s):
        for k, v in (("_xyz", "xyz"), ("_features_dc", "dc"), ("_features_rest", "rest"), ("_opacity", "opacity"),
                     ("_scaling", "scaling"), ("_rotation", "rotation")):
            setattr(self, k, s[v].clone().requires_grad_())
        self._degrees = s["degrees"]

    leaves = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: F.normalize(self._rotation))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))


def test_render_end_to_end_gradients_and_determinism():
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    s = scene("small_mixed")
    cam = Cam(s)
    lam = 0.1
    runs = []
    for _ in range(2):
        pc = Model(s)
        out = r3dgs_render.render(cam, pc, Pipe, s["bg"], lambda_sh_sparsity=lam)
        assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii", "FPS"}
        (out["render"] * s["dL"]).sum().backward()
        runs.append((out["render"].detach().clone(), out["radii"].clone(), out["viewspace_points"].grad.clone(),
                     [getattr(pc, k).grad.clone() for k in Model.leaves]))
    for a, b in zip(runs[0][3] + [runs[0][0], runs[0][2]], runs[1][3] + [runs[1][0], runs[1][2]]):
        assert torch.equal(a, b), "not deterministic run to run"
    # the same numbers as the direct calls (items 5-6 hold those to the existing path)
    s2 = dict(s)
    c = s["cam"]
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    fwd = _C.rasterize_gaussian_params(s["bg"], s["xyz"], s["dc"], s["rest"], s["degrees"], s["opacity"], s["scaling"],
                                       s["rotation"], 1.0, s["vm"], s["pm"], tx, ty, s["H"], s["W"], s["cp"], False, False)
    g = _C.rasterize_gaussian_params_backward(s["bg"], s["xyz"], fwd[2], s["dc"], s["rest"], s["degrees"], s["opacity"],
                                              s["scaling"], s["rotation"], 1.0, s["vm"], s["pm"], tx, ty, s["dL"], s["cp"],
                                              fwd[3], fwd[0], fwd[4], fwd[5], lam, False)
    image, radii, m2d, grads = runs[0]
    assert torch.equal(image, fwd[1]) and torch.equal(radii, fwd[2]) and torch.equal(m2d, g[0])
    for got, want in zip(grads, (g[2], g[3], g[4], g[1], g[5], g[6])):
        assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(out["visibility_filter"], radii > 0)
    # a route the fused path does not cover goes through the existing package and agrees to rounding
    pc = Model(s)
    Pipe2 = type("Pipe2", (), dict(debug=False, compute_cov3D_python=False, convert_SHs_python=False))
    over = torch.rand(s["P"], 3, device="cuda")
    out2 = r3dgs_render.render(cam, pc, Pipe2, s["bg"], override_color=over)
    assert out2["render"].shape == image.shape and torch.equal(out2["radii"], radii)


def test_gradients_against_float64_autograd():
    """2 k Gaussians: the fused path's gradients of the RAW leaves against float64 autograd of oracle/torch_ref.py composed
    with torch's exp / F.normalize, at the parity suite's per-tensor bar 1e-4 * max|ref|.  Pixels where the fp32 forward's
    discrete decisions are threshold-ambiguous are left out of the upstream gradient for both sides, as that suite does."""
    import r3dgs_render
    from oracle import oracle as orc
    from oracle import torch_ref as tr
    W, H, P = 96, 64, 2000
    cam = ss.make_camera(W, H, 80.0, 2)
    g = ss.make_gaussians(P, cam, seed=4, degree_mode="mixed", scale_mu=0.08)
    rng = np.random.default_rng(9)
    rot_raw = (g["rotations"] * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)
    log_s = np.log(g["scales"]).astype(np.float32)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    s = dict(W=W, H=H, P=P, cam=cam, xyz=_dev(g["means3D"]), dc=_dev(g["sh"][:, :1]), rest=_dev(g["sh"][:, 1:]),
             opacity=_dev(g["opacity"]), scaling=_dev(log_s), rotation=_dev(rot_raw), degrees=_dev(g["degrees"]), bg=_dev(bg),
             vm=_dev(cam.world_view_transform), pm=_dev(cam.full_proj_transform), cp=_dev(cam.camera_center))
    # ambiguity mask from the fp32 oracle on the activated values
    q32 = (rot_raw / np.linalg.norm(rot_raw.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    ref = orc.forward(bg, g["means3D"], None, g["opacity"], np.exp(log_s), q32, 1.0, None, cam.world_view_transform,
                      cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                      want_ambig=True, ambig_rel=1e-4)
    dl = ss.upstream_grad(W, H, seed=1) * (W * H)
    dl.reshape(3, -1)[:, ref["ambig"].reshape(-1) != 0] = 0.0
    s["dL"] = _dev(dl)
    lam = 0.05
    cm = Cam(s)
    cm.FoVx, cm.FoVy = 2 * math.atan(cam.tanfovx), 2 * math.atan(cam.tanfovy)
    pc = Model(s)
    out = r3dgs_render.render(cm, pc, Pipe, s["bg"], lambda_sh_sparsity=lam)
    (out["render"] * s["dL"]).sum().backward()
    # float64 autograd
    D = torch.float64
    T = lambda a: torch.tensor(np.asarray(a), dtype=D)
    leaves = dict(xyz=T(g["means3D"]), dc=T(g["sh"][:, :1]), rest=T(g["sh"][:, 1:]), opacity=T(g["opacity"]), scaling=T(log_s),
                  rotation=T(rot_raw))
    for v in leaves.values():
        v.requires_grad_()
    color, radii, sparsity = tr.render(leaves["xyz"], leaves["opacity"], torch.exp(leaves["scaling"]),
                                       F.normalize(leaves["rotation"]), torch.cat((leaves["dc"], leaves["rest"]), dim=1),
                                       torch.tensor(g["degrees"]), T(cam.world_view_transform), T(cam.full_proj_transform),
                                       T(cam.camera_center), T(bg), W, H, cam.tanfovx, cam.tanfovy, lambda_sh_sparsity=lam)
    ((color * T(dl)).sum() + sparsity).backward()
    assert np.array_equal(radii.numpy(), out["radii"].cpu().numpy())
    for mine, theirs in (("_xyz", "xyz"), ("_features_dc", "dc"), ("_features_rest", "rest"), ("_opacity", "opacity"),
                         ("_scaling", "scaling"), ("_rotation", "rotation")):
        want = leaves[theirs].grad.numpy()
        got = getattr(pc, mine).grad.cpu().numpy().astype(np.float64).reshape(want.shape)
        e = np.abs(got - want).max() / np.abs(want).max()
        print(f"{theirs}: max err / max|ref| = {e:.2e}")
        assert e <= 1e-4, (theirs, e)


def test_loop_with_loss_and_adam_fused_pass_equals_exact_pass():
    """50 steps of render + r3dgs_loss + r3dgs_optim over the six raw leaves with a changing P: every step's fused pass
    (default settings: asynchronous, strict) equals the exact-size pass bit for bit."""
    import r3dgs_loss
    import r3dgs_optim
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    s = dict(scene("small_mixed"))
    cam = Cam(s)
    pc = Model(s)
    with torch.no_grad():
        gt = r3dgs_render.render(cam, pc, Pipe, s["bg"])["render"].clone()
        gt = (gt + 0.05 * torch.rand_like(gt)).clamp(0, 1)
    lrs = dict(_xyz=1.6e-4, _features_dc=2.5e-3, _features_rest=1.25e-4, _opacity=0.05, _scaling=5e-3, _rotation=1e-3)

    def make_opt():
        return r3dgs_optim.Adam([{"params": [getattr(pc, k)], "lr": lr, "name": k} for k, lr in lrs.items()], eps=1e-15)
    opt = make_opt()
    PipeDebug = type("PipeDebug", (), dict(debug=True, compute_cov3D_python=False, convert_SHs_python=False))
    gen = torch.Generator(device="cuda").manual_seed(5)
    _C.reserve_forget()
    before = _C.pass_stats()
    for step in range(50):
        lam = 0.1 if step % 3 == 0 else 0.0
        opt.zero_grad(set_to_none=True)
        out = r3dgs_render.render(cam, pc, Pipe, s["bg"], lambda_sh_sparsity=lam)
        r3dgs_loss.l1_dssim(out["render"], gt, 0.2)[0].backward()
        got = [getattr(pc, k).grad.clone() for k in Model.leaves] + [out["viewspace_points"].grad.clone()]
        for k in Model.leaves:
            getattr(pc, k).grad = None
        outx = r3dgs_render.render(cam, pc, PipeDebug, s["bg"], lambda_sh_sparsity=lam)   # debug: the exact-size path
        r3dgs_loss.l1_dssim(outx["render"], gt, 0.2)[0].backward()
        assert torch.equal(out["render"], outx["render"]) and torch.equal(out["radii"], outx["radii"]), step
        want = [getattr(pc, k).grad for k in Model.leaves] + [outx["viewspace_points"].grad]
        for a, b in zip(got, want):
            assert torch.equal(a, b) and torch.isfinite(a).all(), step
        opt.step()
        if step % 10 == 9:   # densify / prune stand-in: clone 6 %, drop 3 %, new optimiser state
            with torch.no_grad():
                P = pc._xyz.shape[0]
                idx = torch.randperm(P, generator=gen, device="cuda")
                clone, keep = idx[: P * 6 // 100], idx[P * 3 // 100:]
                for k in Model.leaves:
                    p = getattr(pc, k)
                    setattr(pc, k, torch.cat([p[keep], p[clone]]).contiguous().requires_grad_())
                pc._degrees = torch.cat([pc._degrees[keep], pc._degrees[clone]]).contiguous()
            opt = make_opt()
    after = _C.pass_stats()
    assert after["reserved_passes"] - before["reserved_passes"] >= 40, "the loop did not run on the asynchronous path"


def test_no_joined_sh_tensor_at_500k():
    """A fused forward + backward allocates less than one [P,16,3] fp32 tensor beyond the blobs, the image and the seven
    gradient outputs."""
    from diff_gaussian_rasterization import _C
    import diff_gaussian_rasterization as dgr
    s = scene("metric")
    P, W, H = s["P"], s["W"], s["H"]
    c = s["cam"]
    rs = dgr.GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, s["bg"], 1.0, s["vm"], s["pm"], 3, s["cp"], False, False)
    leaves = [s[k].clone().requires_grad_() for k in ("xyz", "dc", "rest", "opacity", "scaling", "rotation")]

    def run():
        m2d = torch.zeros_like(leaves[0], requires_grad=True) + 0
        m2d.retain_grad()
        color, radii = dgr.rasterize_gaussian_params(leaves[0], m2d, leaves[1], leaves[2], s["degrees"], leaves[3], leaves[4],
                                                     leaves[5], rs, 0.0)
        (color * s["dL"]).sum().backward()
        return color
    run()   # learns the reservation; allocator warm
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    nr = fused_forward(_C, s, False, None)[0]
    blobs = sum(int(t.numel()) for t in fused_forward(_C, s, False, None)[3:6])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    f = 4
    accounted = (blobs + 3 * H * W * f            # state blobs, image
                 + P * 4                           # radii
                 + 2 * P * 3 * f                   # means2D and its zero source
                 + 2 * 3 * H * W * f               # color * dL and the upstream gradient of the image
                 + P * (3 + 3 + 1 + 3 + 45 + 3 + 4) * f)   # the seven gradient outputs
    joined = P * 16 * 3 * f
    print(f"\npeak growth {grew / 1e6:.1f} MB, accounted {accounted / 1e6:.1f} MB, one joined SH tensor {joined / 1e6:.1f} MB")
    assert grew - accounted < joined, (grew, accounted, joined)
    assert nr.capacity > 0
