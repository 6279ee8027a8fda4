"""GPU checks of the anti-aliasing unit (reduced-3dgs_amd/r3dgs_mip.py, csrc/mip.hip) against the float64 restatement
tests/mip_ref.py, at the project's bars:
    values      sigmoid(raw_eff) and exp(log_scale_eff) within 1e-5 of the reference; filter_3d within 1e-5 RELATIVE
    gradients   every tensor within 1e-4 * max|ref|
    f = 0       gives the inputs back bit for bit
    determinism two runs, and a run captured in torch.cuda.graph, give the same bits
and end to end: render(antialiasing=True, filter_3d=f) against a plain render of a copy of the model that holds the ops' outputs.
Rows the reference calls ambiguous (at most 1 % of a test's rows) are left out.  P in {1, 63, 1000, 4097}: ragged tails on a
64-lane wave and on a 256-thread block, more than one block; V in {1, 3, 70}: 70 is more than the kernel's staging chunk of 64
camera rows.

filter_3d and 1e-5 relative: the kernel evaluates the view depth in double from the fp32 inputs (csrc/mip_math.h
mip_filter_valid) and rounds it to fp32 once, then divides by the focal length and multiplies by sqrt(0.2) in fp32 -- three
roundings of 2^-24 = 6e-8 each, 1.8e-7 relative in all -- so the bar the issue sets holds as it stands and the fall-back bar it
allows (four fp32 products in z) is not needed.  Measured worst figures: profiles/mip_gpu_tests.txt."""
import math
import types

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import mip_cases as cases
from tests import mip_ref as ref
from tests import test_mip_cpu as host

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (1, 63, 1000, 4097)
VALUE_BAR, GRAD_BAR = host.VALUE_BAR, host.GRAD_BAR


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _settings(s, mod=1.0):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(cases.H, cases.W, cases.TAN_FOVX, cases.TAN_FOVY, None, mod, _dev(s["viewmatrix"]), None, 3,
                                         None, False, False)


def _run_opacity(s, form, g, mod=1.0):
    """The autograd function and the rho-returning call on one scene -> what tests/test_mip_cpu.compare_opacity takes."""
    import r3dgs_mip as mip
    sk, rk, ck, raw = host.FORMS[form]
    rs = _settings(s, mod)
    leaf = lambda k: None if k is None else _dev(s[k]).requires_grad_()
    m, o, sc, rot, cov = leaf("means3D"), leaf("opacities"), leaf(sk), leaf(rk), leaf(ck)
    raw_eff = mip.antialias_opacity(m, o, sc, rot, cov, rs, raw=bool(raw))
    raw_eff.backward(_dev(g))
    raw_eff2, rho = mip.antialias_rho(m, o, sc, rot, cov, rs, raw=bool(raw))
    assert np.array_equal(_bits(raw_eff), _bits(raw_eff2)), "two runs, different bits"
    P = len(g)
    got = {"raw_eff": raw_eff.detach().cpu().numpy(), "rho": rho.cpu().numpy(), "d_o": o.grad.cpu().numpy(), "d_means": m.grad.cpu().numpy()}
    if cov is None:
        got["d_scales"], got["d_rot"] = sc.grad.cpu().numpy(), rot.grad.cpu().numpy()
    else:
        got["d_cov"] = cov.grad.cpu().numpy()
    assert got["raw_eff"].shape == (P, 1) and got["rho"].shape == (P,)
    return got


@pytest.mark.parametrize("form", list(host.FORMS))
@pytest.mark.parametrize("P", SIZES)
def test_compensation_values_and_gradients(P, form):
    s = cases.scene(P, seed=P)
    g = np.random.default_rng(P).normal(0, 1, (P, 1)).astype(F32)
    mod = 0.7 if P == 63 else 1.0
    got = _run_opacity(s, form, g, mod)
    worst = host.compare_opacity(got, s, form, g, mod)
    print(f"mip: compensation {form} P={P}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    behind = s["kind"] == 0
    assert np.array_equal(got["raw_eff"][behind], s["opacities"][behind]) and np.array_equal(got["d_o"][behind], g[behind])
    assert not got["d_means"][behind].any()


def test_compensation_skips_the_outputs_nobody_asks_for():
    import r3dgs_mip as mip
    s = cases.scene(1000, 1)
    m, o = _dev(s["means3D"]), _dev(s["opacities"]).requires_grad_()
    raw_eff = mip.antialias_opacity(m, o, _dev(s["scales"]), _dev(s["rotations"]), None, _settings(s))
    g = torch.ones_like(raw_eff)
    (d_o,) = torch.autograd.grad(raw_eff, [o], g)
    full = _run_opacity(s, "activated", np.ones((1000, 1), F32))
    assert np.array_equal(_bits(d_o), full["d_o"].view(np.uint32)), "the gradient of o does not depend on which outputs are written"
    empty = mip.antialias_opacity(m[:0], o[:0], _dev(s["scales"])[:0], _dev(s["rotations"])[:0], None, _settings(s))
    assert empty.shape == (0, 1)


@pytest.mark.parametrize("P", SIZES)
def test_filtered_parameters(P):
    import r3dgs_mip as mip
    s, f = cases.scene(P, seed=P + 1), cases.filter_values(P, seed=P)
    rng = np.random.default_rng(P)
    g_ls, g_o = rng.normal(0, 1, (P, 3)).astype(F32), rng.normal(0, 1, (P, 1)).astype(F32)
    ls, o, fd = _dev(s["scaling_raw"]).requires_grad_(), _dev(s["opacities"]).requires_grad_(), _dev(f)
    ls_eff, o_eff = mip.filtered_parameters(ls, o, fd)
    torch.autograd.backward([ls_eff, o_eff], [_dev(g_ls), _dev(g_o)])
    zero = f[:, 0] == 0
    assert np.array_equal(_bits(ls_eff)[zero], s["scaling_raw"].view(np.uint32)[zero]), "f = 0: the inputs, bit for bit"
    assert np.array_equal(_bits(o_eff)[zero], s["opacities"].view(np.uint32)[zero])
    assert np.array_equal(_bits(ls.grad)[zero], g_ls.view(np.uint32)[zero]) and np.array_equal(_bits(o.grad)[zero], g_o.view(np.uint32)[zero])
    all_zero = mip.filtered_parameters(ls.detach(), o.detach(), torch.zeros_like(fd))
    assert np.array_equal(_bits(all_zero[0]), s["scaling_raw"].view(np.uint32)) and np.array_equal(_bits(all_zero[1]), s["opacities"].view(np.uint32))
    rls, ro = ref.leaves(s["scaling_raw"], s["opacities"])
    want_ls, want_o = ref.filtered(rls, ro, ref._t(f))
    w_dls, w_do = ref.vjp([want_ls, want_o], [g_ls, g_o], [rls, ro])
    e_s = np.abs(np.exp(ls_eff.detach().cpu().numpy().astype(np.float64)) - np.exp(want_ls.detach().numpy())).max()
    e_o = np.abs(host._sig(o_eff.detach().cpu().numpy()) - host._sig(want_o.detach().numpy())).max()
    e_dls = np.abs(ls.grad.cpu().numpy() - w_dls.numpy()).max() / np.abs(w_dls.numpy()).max()
    e_do = np.abs(o.grad.cpu().numpy() - w_do.numpy()).max() / np.abs(w_do.numpy()).max()
    print(f"mip: filtered P={P}: exp(ls_eff) {e_s:.2e}, sigmoid(raw_eff) {e_o:.2e}, d_ls {e_dls:.2e}, d_o {e_do:.2e}")
    assert e_s <= VALUE_BAR and e_o <= VALUE_BAR and e_dls <= GRAD_BAR and e_do <= GRAD_BAR


@pytest.mark.parametrize("V", (1, 3, 70))
@pytest.mark.parametrize("P", SIZES)
def test_filter_3d(P, V):
    import r3dgs_mip as mip
    s, cams = cases.scene(P, seed=P + 2), cases.cameras(V)
    xyz, table = _dev(s["means3D"]), _dev(cams)
    got = mip.filter_3d(xyz, table)
    again = mip.filter_3d(xyz, table)
    assert got.shape == (P, 1) and np.array_equal(_bits(got), _bits(again)), "two runs, different bits"
    want, amb = ref.filter3d(s["means3D"], cams)
    want, keep = want.numpy(), ~amb.numpy()
    assert (~keep).mean() <= ref.MAX_AMBIGUOUS
    have, want = got.cpu().numpy()[keep], want[keep]
    seen = want > 0   # all of them, unless no camera sees any Gaussian of the scene (P = 1: the one Gaussian may lie behind them)
    assert seen.all() or (P == 1 and not have.any())
    rel = np.abs(have[seen] - want[seen]) / want[seen]
    print(f"mip: filter_3d P={P} V={V}: worst relative error {rel.max() if rel.size else 0.0:.2e} (bar 1e-5)")
    assert (rel <= 1e-5).all()
    far = _dev((s["means3D"] + F32(1e4)).astype(F32))
    assert not mip.filter_3d(far, table).any(), "no Gaussian is valid in any camera: every d is 0"


def test_filter_3d_from_camera_objects_and_the_portrait_pair():
    import r3dgs_mip as mip
    s = cases.scene(1000, 9)
    cams = cases.cameras(2)
    assert (cams[0, 18], cams[0, 19], cams[1, 18], cams[1, 19]) == (64, 48, 48, 64) and cams[0, 16] != cams[0, 17]
    objs = [types.SimpleNamespace(world_view_transform=_dev(c[:16].reshape(4, 4)), FoVx=2 * math.atan(c[18] / (2 * c[16])),
                                  FoVy=2 * math.atan(c[19] / (2 * c[17])), image_width=int(c[18]), image_height=int(c[19])) for c in cams]
    table = mip.pack_cameras(objs, "cuda")
    assert np.allclose(table.cpu().numpy(), cams, rtol=1e-6)
    a, b = mip.filter_3d(_dev(s["means3D"]), objs), mip.filter_3d(_dev(s["means3D"]), table)
    assert np.array_equal(_bits(a), _bits(b))


def test_graph_capture_gives_the_same_bits():
    import r3dgs_mip as mip
    P = 4097
    s, f, cams = cases.scene(P, 4), cases.filter_values(P, 4), cases.cameras(70)
    rs = _settings(s)
    m, o = _dev(s["means3D"]).requires_grad_(), _dev(s["opacities"]).requires_grad_()
    ls, rot = _dev(s["scaling_raw"]).requires_grad_(), _dev(s["rotation_raw"]).requires_grad_()
    fd, table = _dev(f), _dev(cams)
    g = _dev(np.random.default_rng(4).normal(0, 1, (P, 1)).astype(F32))

    def step():
        f3 = mip.filter_3d(m, table)
        ls_eff, o_eff = mip.filtered_parameters(ls, o, fd)
        raw_eff = mip.antialias_opacity(m, o_eff, ls_eff, rot, None, rs, raw=True)
        grads = torch.autograd.grad(raw_eff, [m, o, ls, rot], g)
        return (f3, ls_eff, raw_eff) + tuple(grads)
    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert np.array_equal(_bits(a), _bits(b)), "the captured run differs from the eager one"


# ---- end to end ---------------------------------------------------------------------------------------------------------

class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def _scene_model(P=2000, seed=3):
    cam = ss.Camera(64, 48, 58.0, 66.0, ss.rot_xyz(0.05, -0.08, 0.03), np.array([0.1, -0.05, 0.2]))
    g = ss.make_gaussians(P, cam, seed=seed, degree_mode="mixed", scale_mu=0.02, scale_sigma=1.2)
    rng = np.random.default_rng(seed)
    camera = types.SimpleNamespace(FoVx=cam.FoVx, FoVy=cam.FoVy, image_height=48, image_width=64,
                                   world_view_transform=_dev(cam.world_view_transform), full_proj_transform=_dev(cam.full_proj_transform),
                                   camera_center=_dev(cam.camera_center))
    arrays = {"_xyz": g["means3D"], "_features_dc": g["sh"][:, :1], "_features_rest": g["sh"][:, 1:], "_opacity": g["opacity"],
              "_scaling": np.log(g["scales"]), "_rotation": g["rotations"] * 10.0 ** rng.uniform(-0.5, 0.5, (P, 1)).astype(F32)}

    def model(**replace):
        pc = types.SimpleNamespace(active_sh_degree=3, max_sh_degree=3, _degrees=_dev(g["degrees"]))
        for name, a in arrays.items():
            t = replace[name] if name in replace else _dev(a.astype(F32))
            setattr(pc, name, torch.nn.Parameter(t.detach().clone()))
        return pc
    return camera, model, arrays


def test_render_with_both_filters_equals_a_plain_render_of_the_filtered_model():
    import r3dgs_mip as mip
    import r3dgs_render
    camera, model, arrays = _scene_model()
    P = 2000
    bg = _dev(np.array([0.1, 0.2, 0.3], F32))
    aux = ("depth", "alpha", "median_depth")
    dl = _dev(ss.upstream_grad(64, 48, seed=2) * (64 * 48))
    pc = model()
    f = mip.filter_3d(pc._xyz, mip.pack_cameras([camera], "cuda"))
    assert f.shape == (P, 1) and (f > 0).all()
    out = r3dgs_render.render(camera, pc, _Pipe, bg, antialiasing=True, filter_3d=f, aux=aux)
    (out["render"] * dl).sum().backward()
    # a copy of the model whose _scaling / _opacity hold the ops' detached outputs, rendered plainly
    rs = r3dgs_render._settings(camera, pc, _Pipe, bg, 1.0)
    with torch.no_grad():
        s_eff, o_eff = mip.filtered_parameters(pc._scaling, pc._opacity, f)
        o_aa = mip.antialias_opacity(pc._xyz, o_eff, s_eff, pc._rotation, None, rs, raw=True)
    assert not torch.equal(o_aa, pc._opacity) and not torch.equal(s_eff, pc._scaling)
    plain = model(_scaling=s_eff, _opacity=o_aa)
    out2 = r3dgs_render.render(camera, plain, _Pipe, bg, aux=aux)
    (out2["render"] * dl).sum().backward()
    assert int((out["radii"] > 0).sum()) > P // 4
    for key in ("render", "radii") + aux:
        assert torch.equal(out[key], out2[key]), f"{key} differs from the plain render of the filtered model"
    # backward: the plain render's gradients of the two leaves, pushed through the float64 vector-Jacobian product of the maps
    xyz, ls, o, rot = ref.leaves(arrays["_xyz"], arrays["_scaling"].astype(F32), arrays["_opacity"], pc._rotation.detach().cpu().numpy())
    ls_eff, o_eff64 = ref.filtered(ls, o, ref._t(f))
    raw_eff, _, amb = ref.opacity(xyz, o_eff64, ls_eff, rot, None, ref._t(camera.world_view_transform), math.tan(camera.FoVx * 0.5),
                                  math.tan(camera.FoVy * 0.5), 64, 48, 1.0, raw=True)
    keep = ~amb.numpy()
    assert (~keep).mean() <= ref.MAX_AMBIGUOUS
    G_o = plain._opacity.grad.cpu().numpy().astype(np.float64) * keep[:, None]
    d_xyz, d_ls, d_o, d_rot = ref.vjp([ls_eff, raw_eff], [plain._scaling.grad, G_o], [xyz, ls, o, rot])
    want = {"_xyz": plain._xyz.grad.cpu().numpy() + d_xyz.numpy(), "_rotation": plain._rotation.grad.cpu().numpy() + d_rot.numpy(),
            "_scaling": d_ls.numpy(), "_opacity": d_o.numpy(), "_features_dc": plain._features_dc.grad.cpu().numpy(),
            "_features_rest": plain._features_rest.grad.cpu().numpy()}
    figures = []
    for name, w in want.items():
        got = getattr(pc, name).grad.cpu().numpy().astype(np.float64)
        top = np.abs(w[keep]).max()
        err = np.abs(got[keep] - w[keep]).max()
        figures.append(f"{name} {err / top:.2e}")
        assert top > 0 and err <= GRAD_BAR * top, f"{name}: error {err:.3g}, bar {GRAD_BAR} * {top:.3g}"
    print("mip: end to end, gradient errors / max|ref| (bar 1e-4): " + ", ".join(figures))


def test_render_with_one_filter_each_and_with_aux_grad():
    import r3dgs_mip as mip
    import r3dgs_render
    camera, model, _ = _scene_model(P=500, seed=6)
    bg = _dev(np.array([0.0, 0.0, 0.0], F32))
    pc = model()
    f = mip.filter_3d(pc._xyz, mip.pack_cameras([camera], "cuda"))
    rs = r3dgs_render._settings(camera, pc, _Pipe, bg, 1.0)
    base = r3dgs_render.render(camera, pc, _Pipe, bg)
    with torch.no_grad():
        only_aa = r3dgs_render.render(camera, pc, _Pipe, bg, antialiasing=True)
        o_aa = mip.antialias_opacity(pc._xyz, pc._opacity, pc._scaling, pc._rotation, None, rs, raw=True)
        assert torch.equal(only_aa["render"], r3dgs_render.render(camera, model(_opacity=o_aa), _Pipe, bg)["render"])
        only_f = r3dgs_render.render(camera, pc, _Pipe, bg, filter_3d=f)
        s_eff, o_eff = mip.filtered_parameters(pc._scaling, pc._opacity, f)
        assert torch.equal(only_f["render"], r3dgs_render.render(camera, model(_scaling=s_eff, _opacity=o_eff), _Pipe, bg)["render"])
        assert not torch.equal(only_aa["render"], base["render"]) and not torch.equal(only_f["render"], base["render"])
        zero = r3dgs_render.render(camera, pc, _Pipe, bg, filter_3d=torch.zeros_like(f))
        assert torch.equal(zero["render"], base["render"]), "f = 0 renders the model itself"
        baked = mip.bake(model(), f)
        assert torch.equal(baked._scaling, s_eff) and torch.equal(baked._opacity, o_eff) and isinstance(baked._scaling, torch.nn.Parameter)
    # a loss on an attached aux map reaches the raw parameters through both maps
    out = r3dgs_render.render(camera, pc, _Pipe, bg, antialiasing=True, filter_3d=f, aux=("alpha",), aux_grad=True)
    out["alpha"].sum().backward()
    assert pc._opacity.grad is not None and pc._opacity.grad.abs().sum() > 0 and pc._scaling.grad.abs().sum() > 0
    assert torch.isfinite(pc._opacity.grad).all() and torch.isfinite(pc._scaling.grad).all() and torch.isfinite(pc._xyz.grad).all()
