"""CPU checks of the anti-aliasing unit (reduced-3dgs_amd/r3dgs_mip.py, csrc/mip.hip, csrc/mip_math.h, include/r3dgs_mip.h):
the float64 restatement (tests/mip_ref.py) is pinned by hand-worked cases; the per-Gaussian kernel arithmetic runs on the host
through a test shim and is held to the restatement -- values and every partial derivative, with needles, sub-pixel Gaussians on
the floor, f = 0, Gaussians behind the near plane and the cancelled forms at o = +-15; the same shim runs as a stand-alone
program, plain and under ASan/UBSan; the ABI rows, every refusal, and render()'s keyword handling with a fake model and no
launch.  No GPU needed."""
import ctypes as C
import inspect
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import hostcheck_build as hb
from tests import mip_cases as cases
from tests import mip_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_mip", "hostcheck_mip.hip")
SO = os.path.join(HERE, "hostcheck_mip", "libhostcheck_mip.so")
F32 = np.float32
VALUE_BAR, GRAD_BAR = 1e-5, 1e-4   # the GPU tests' bars


def _shim():
    lib = hb.build_shim(SRC, SO, hb.EXACT, "hipcc not available to build the anti-aliasing host-check shim")
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    lib.hc_mip_opacity.argtypes = [i, vp, vp, vp, vp, vp, i, vp, f, f, i, i, f, vp, vp]
    lib.hc_mip_opacity_bwd.argtypes = [i, vp, vp, vp, vp, vp, i, vp, f, f, i, i, f, vp, vp, vp, vp, vp, vp]
    lib.hc_mip_filter3d.argtypes = [i, i, vp, vp, vp]
    lib.hc_mip_filtered.argtypes = [i, vp, vp, vp, vp, vp]
    lib.hc_mip_filtered_bwd.argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
    lib.hc_mip_cov2d_both.argtypes = [vp, vp, vp, vp, f, f, i, i, f, vp, vp]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


FORMS = {"activated": ("scales", "rotations", None, 0), "raw": ("scaling_raw", "rotation_raw", None, 1),
         "cov3D": (None, None, "cov3D", 0)}


def _host_opacity(lib, s, form, g, mod=1.0):
    sk, rk, ck, raw = FORMS[form]
    P = len(s["means3D"])
    sc, rot, cov = (s[k] if k else None for k in (sk, rk, ck))
    out = {"raw_eff": np.zeros((P, 1), F32), "rho": np.zeros(P, F32), "d_o": np.zeros((P, 1), F32), "d_means": np.zeros((P, 3), F32),
           "d_scales": np.zeros((P, 3), F32), "d_rot": np.zeros((P, 4), F32), "d_cov": np.zeros((P, 6), F32)}
    view = np.ascontiguousarray(s["viewmatrix"].reshape(16))
    lib.hc_mip_opacity(P, _p(s["means3D"]), _p(sc), _p(rot), _p(cov), _p(s["opacities"]), raw, _p(view), cases.TAN_FOVX,
                       cases.TAN_FOVY, cases.W, cases.H, mod, _p(out["raw_eff"]), _p(out["rho"]))
    lib.hc_mip_opacity_bwd(P, _p(s["means3D"]), _p(sc), _p(rot), _p(cov), _p(s["opacities"]), raw, _p(view), cases.TAN_FOVX,
                           cases.TAN_FOVY, cases.W, cases.H, mod, _p(g), _p(out["d_o"]), _p(out["d_means"]), _p(out["d_scales"]),
                           _p(out["d_rot"]), _p(out["d_cov"]))
    return out


def ref_opacity(s, form, g, mod=1.0):
    """-> values, gradients and the ambiguous rows of the float64 restatement for one scene and one input form."""
    sk, rk, ck, raw = FORMS[form]
    m, o, sc, rot, cov = ref.leaves(s["means3D"], s["opacities"], s[sk] if sk else None, s[rk] if rk else None, s[ck] if ck else None)
    raw_eff, rho, amb = ref.opacity(m, o, sc, rot, cov, ref._t(s["viewmatrix"]), cases.TAN_FOVX, cases.TAN_FOVY, cases.W, cases.H, mod,
                                    raw=bool(raw))
    keep = (~amb).to(ref.F64).reshape(-1, 1)
    d_m, d_o, d_s, d_r, d_c = ref.vjp([raw_eff], [ref._t(g).reshape(-1, 1) * keep], [m, o, sc, rot, cov])
    grads = {"d_o": d_o, "d_means": d_m, "d_scales": d_s, "d_rot": d_r, "d_cov": d_c}
    return raw_eff.detach().numpy(), rho.detach().numpy(), amb.numpy(), {k: v.numpy() for k, v in grads.items() if v is not None}


def compare_opacity(got, s, form, g, mod=1.0):
    """Holds a set of outputs to the restatement at the issue's bars -> the worst figures."""
    raw_eff, rho, amb, grads = ref_opacity(s, form, g, mod)
    keep = ~amb
    assert amb.mean() <= ref.MAX_AMBIGUOUS, f"{amb.sum()} ambiguous rows of {amb.size}: more than 1 %"
    worst = {"value": float(np.abs(_sig(got["raw_eff"][keep]) - _sig(raw_eff[keep])).max()) if keep.any() else 0.0}
    if "rho" in got:
        worst["rho"] = float(np.abs(got["rho"][keep] - rho[keep]).max()) if keep.any() else 0.0
        assert worst["rho"] <= VALUE_BAR
    assert worst["value"] <= VALUE_BAR, worst
    for name, want in grads.items():
        if name not in got:
            continue
        top = np.abs(want[keep]).max() if keep.any() else 0.0
        err = float(np.abs(got[name][keep].astype(np.float64) - want[keep]).max()) if keep.any() else 0.0
        worst[name] = err / top if top > 0 else err
        assert err <= GRAD_BAR * top + 1e-300, f"{form}: {name}: error {err:.3g}, bar {GRAD_BAR} * {top:.3g}"
    return worst


# ---- the restatement, pinned by hand -----------------------------------------------------------------------------------------

def test_reference_is_pinned_by_hand_worked_cases():
    eye = torch.eye(4, dtype=ref.F64)
    fx = ref.view_constants(0.5, 0.5, 100, 100)["fx"]
    assert fx == 100.0
    # an isotropic Gaussian on the optical axis: C = (f s / z)^2 I
    for s, z in ((0.01, 2.0), (0.2, 5.0), (1e-4, 3.0)):
        a = (fx * s / z) ** 2
        raw_eff, rho, amb = ref.opacity(torch.tensor([[0.0, 0.0, z]], dtype=ref.F64), torch.tensor([[0.3]], dtype=ref.F64),
                                        torch.full((1, 3), s, dtype=ref.F64), torch.tensor([[1.0, 0, 0, 0]], dtype=ref.F64), None, eye,
                                        0.5, 0.5, 100, 100)
        want = math.sqrt(max(0.000025, a * a / (a + 0.3) ** 2))
        assert float(rho) == pytest.approx(want, rel=1e-12) and not bool(amb)
        assert float(torch.sigmoid(raw_eff)) == pytest.approx(_sig(0.3) * want, rel=1e-12)
    # behind the near plane: the opacity itself
    raw_eff, rho, _ = ref.opacity(torch.tensor([[0.0, 0.0, 0.1]], dtype=ref.F64), torch.tensor([[0.3]], dtype=ref.F64),
                                  torch.full((1, 3), 0.1, dtype=ref.F64), torch.tensor([[1.0, 0, 0, 0]], dtype=ref.F64), None, eye, 0.5,
                                  0.5, 100, 100)
    assert float(raw_eff) == 0.3 and float(rho) == 1.0
    # the 3D filter applied: s = (1, 2, 3), f = 2
    ls = torch.log(torch.tensor([[1.0, 2.0, 3.0]], dtype=ref.F64))
    ls_eff, raw_eff = ref.filtered(ls, torch.tensor([[-0.4]], dtype=ref.F64), torch.tensor([[2.0]], dtype=ref.F64))
    assert torch.allclose(torch.exp(ls_eff) ** 2, torch.tensor([[5.0, 8.0, 13.0]], dtype=ref.F64), rtol=1e-13)
    assert float(torch.sigmoid(raw_eff)) == pytest.approx(_sig(-0.4) * math.sqrt(36.0 / (5 * 8 * 13)), rel=1e-13)
    # the filter itself: two cameras on the axis at distance 2 and 5 of a point; focal 100 and 80
    cam = lambda tz, f: np.concatenate([np.eye(4).reshape(16), [f, f, 100, 100]]) + np.eye(20)[14] * tz
    f3, amb = ref.filter3d(np.array([[0.0, 0.0, 0.0], [50.0, 0.0, 0.0]]), np.stack([cam(2.0, 100.0), cam(5.0, 80.0)]))
    assert f3[:, 0].tolist() == pytest.approx([2.0 / 100 * math.sqrt(0.2)] * 2, rel=1e-13), "the unseen point takes the largest d"
    assert not amb.any()


# ---- mip_math.h on the host -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("P,seed,mod", [(1000, 0, 1.0), (63, 1, 1.0), (400, 2, 0.7)])
def test_compensation_values_and_gradients_on_the_host(form, P, seed, mod):
    lib = _shim()
    s = cases.scene(P, seed)
    g = np.random.default_rng(seed).normal(0, 1, (P, 1)).astype(F32)
    got = _host_opacity(lib, s, form, g, mod)
    worst = compare_opacity(got, s, form, g, mod)
    print(f"host, {form}, P = {P}: worst errors {worst}")
    kind = s["kind"]
    assert (got["rho"][kind == 0] == 1).all() and np.array_equal(got["raw_eff"][kind == 0], s["opacities"][kind == 0])
    assert np.array_equal(got["d_o"][kind == 0], g[kind == 0]) and not got["d_means"][kind == 0].any()
    assert not got["d_scales"][kind == 0].any() and not got["d_rot"][kind == 0].any() and not got["d_cov"][kind == 0].any()
    if P >= 400:
        on_floor = (got["rho"] == F32(0.005)) & (kind != 0)
        assert on_floor.sum() >= P // 40, "the sub-pixel rows sit on the floor"
        assert not got["d_means"][on_floor].any() and not got["d_scales"][on_floor].any(), "below the floor rho is a constant"
        assert (got["rho"][kind == 1] > 0.005).any() and np.isfinite(got["d_rot"]).all()


def test_cancelled_forms_at_large_opacities():
    """d raw_eff / d o = (1 - s) / (1 - p) and d raw_eff / d rho = 1 / (rho (1 - p)) row by row, RELATIVE: a form that divided
    by p (1 - p) would lose every digit at o = 15 and overflow at o = -15 with a small rho."""
    lib = _shim()
    s = cases.scene(600, 5)
    s["opacities"][:] = np.where(np.arange(600) % 2, 15.0, -15.0).reshape(-1, 1).astype(F32)
    g = np.ones((600, 1), F32)
    got = _host_opacity(lib, s, "activated", g)
    raw_eff, rho, amb, grads = ref_opacity(s, "activated", g)
    keep = ~amb
    rel = np.abs(got["d_o"][keep] - grads["d_o"][keep]) / np.abs(grads["d_o"][keep])
    assert rel.max() <= 1e-5, rel.max()
    assert np.abs(got["raw_eff"][keep] - raw_eff[keep]).max() <= 2e-5, "the logits themselves, absolute"
    live = keep & (got["rho"] > 0.005) & (s["kind"] != 0)
    for name in ("d_means", "d_scales", "d_rot"):
        rows = np.abs(grads[name][live]).max(axis=1)
        err = np.abs(got[name][live] - grads[name][live]).max(axis=1)
        assert (err <= 1e-5 * rows + 1e-30).all(), name


def test_the_covariance_is_the_one_the_forward_dilates():
    """cov2d of gauss_math.h (fp32, dilated) against the undilated double covariance of mip_math.h plus 0.3."""
    lib = _shim()
    s = cases.scene(300, 7)
    view = np.ascontiguousarray(s["viewmatrix"].reshape(16))
    seen = 0
    for i in np.flatnonzero((s["kind"] > 2))[:120]:
        fwd, mine = np.zeros(3, F32), np.zeros(3, np.float64)
        lib.hc_mip_cov2d_both(_p(s["means3D"][i]), _p(s["scales"][i]), _p(s["rotations"][i]), _p(view), cases.TAN_FOVX, cases.TAN_FOVY,
                              cases.W, cases.H, 1.0, _p(fwd), _p(mine))
        want = mine + np.array([0.3, 0.0, 0.3])
        size = max(abs(want[0]), abs(want[2]))
        assert np.abs(fwd - want).max() <= 2e-5 * size, (i, fwd, want)
        seen += 1
    assert seen >= 100


@pytest.mark.parametrize("P,seed", [(1000, 0), (63, 3)])
def test_filtered_values_gradients_and_the_copy_branch(P, seed):
    lib = _shim()
    s, f = cases.scene(P, seed), cases.filter_values(P, seed)
    rng = np.random.default_rng(seed)
    g_ls, g_o = rng.normal(0, 1, (P, 3)).astype(F32), rng.normal(0, 1, (P, 1)).astype(F32)
    ls_eff, raw_eff, d_ls, d_o = np.zeros((P, 3), F32), np.zeros((P, 1), F32), np.zeros((P, 3), F32), np.zeros((P, 1), F32)
    lib.hc_mip_filtered(P, _p(s["scaling_raw"]), _p(s["opacities"]), _p(f), _p(ls_eff), _p(raw_eff))
    lib.hc_mip_filtered_bwd(P, _p(s["scaling_raw"]), _p(s["opacities"]), _p(f), _p(g_ls), _p(g_o), _p(d_ls), _p(d_o))
    zero = f[:, 0] == 0
    assert zero.any() and np.array_equal(ls_eff[zero].view(np.uint32), s["scaling_raw"][zero].view(np.uint32))
    assert np.array_equal(raw_eff[zero].view(np.uint32), s["opacities"][zero].view(np.uint32))
    assert np.array_equal(d_ls[zero], g_ls[zero]) and np.array_equal(d_o[zero], g_o[zero])
    ls, o = ref.leaves(s["scaling_raw"], s["opacities"])
    want_ls, want_o = ref.filtered(ls, o, ref._t(f))
    w_dls, w_do = ref.vjp([want_ls, want_o], [g_ls, g_o], [ls, o])
    assert np.abs(np.exp(ls_eff.astype(np.float64)) - np.exp(want_ls.detach().numpy())).max() <= VALUE_BAR
    assert np.abs(_sig(raw_eff) - _sig(want_o.detach().numpy())).max() <= VALUE_BAR
    for got, want in ((d_ls, w_dls.numpy()), (d_o, w_do.numpy())):
        assert np.abs(got - want).max() <= GRAD_BAR * np.abs(want).max()


@pytest.mark.parametrize("P,V", [(1000, 1), (1000, 3), (257, 70), (50, 0)])
def test_filter3d_against_the_reference(P, V):
    lib = _shim()
    s, cams = cases.scene(P, 11), cases.cameras(V)
    got = np.full((P, 1), -7.0, F32)
    lib.hc_mip_filter3d(P, V, _p(s["means3D"]), _p(cams), _p(got))
    want, amb = ref.filter3d(s["means3D"], cams)
    want, keep = want.numpy(), ~amb.numpy()
    assert (~keep).mean() <= ref.MAX_AMBIGUOUS
    if V == 0:
        assert not got.any()
        return
    assert (want > 0).all() and len(np.unique(want)) > min(P, 100) // 2, "most rows are seen by a camera"
    assert (np.abs(got[keep] - want[keep]) <= 1e-5 * want[keep]).all()
    # nobody sees anything: every d is 0
    far = (s["means3D"] + F32(1e4)).astype(F32)
    lib.hc_mip_filter3d(P, V, _p(far), _p(cams), _p(got))
    assert not got.any() and not ref.filter3d(far, cams)[0].numpy().any()


@pytest.mark.parametrize("name,extra", [("hostcheck_mip", ()),
                                        ("hostcheck_mip_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                               "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_stand_alone_program_plain_and_sanitised(name, extra):
    """The shim's own main sweeps every function over its edge inputs.  The second build runs the host side under
    AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    exe = os.path.join(HERE, "hostcheck_mip", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [SRC] + hb._headers()):
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", *hb.EXACT, "-DHOSTCHECK_MIP_MAIN", *extra,
                               "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("checksum ") and out.stdout.strip().endswith("bad 0")


# ---- the ABI and the Python surface ----------------------------------------------------------------------------------------

NAMES = {"r3dgs_mip_opacity", "r3dgs_mip_opacity_backward", "r3dgs_mip_filter3d_workspace_bytes", "r3dgs_mip_filter3d",
         "r3dgs_mip_filtered", "r3dgs_mip_filtered_backward"}


def test_abi_rows_match_the_header():
    from diff_gaussian_rasterization import _C
    from tests import test_abi_table as abi
    protos, rows = abi.header_prototypes(), _C._ABI["required"][1]
    assert NAMES == {n for n in protos if n.startswith("r3dgs_mip")} and NAMES <= set(rows)
    for name in NAMES:
        ret, kinds = protos[name]
        assert abi.ctypes_kind(rows[name][0]) == ret and [abi.ctypes_kind(t) for t in rows[name][1]] == kinds, name
    lib = _C._lib
    assert lib.r3dgs_mip_filter3d_workspace_bytes(0, 3) == 0 and lib.r3dgs_mip_filter3d_workspace_bytes(-1, 3) == 0
    a = lib.r3dgs_mip_filter3d_workspace_bytes(1000, 3)
    assert a == lib.r3dgs_mip_filter3d_workspace_bytes(1000, 3) and a >= 4 * 4 and a % 16 == 0
    import r3dgs_mip
    assert r3dgs_mip.CAMERA_FLOATS == 20 and r3dgs_mip.workspace_bytes(1000, 3) == a


def test_library_refuses_what_the_header_says():
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    err = lambda: lib.r3dgs_last_error().decode()
    n = None
    assert lib.r3dgs_mip_opacity(0, n, n, n, n, n, 0, n, 1.0, 1.0, 8, 8, 1.0, n, n, n) == 0, "P == 0 is valid"
    assert lib.r3dgs_mip_opacity(10, n, n, n, n, n, 0, n, 1.0, 1.0, 8, 8, 1.0, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_mip_opacity_backward(0, n, n, n, n, n, 0, n, 1.0, 1.0, 8, 8, 1.0, n, n, n, n, n, n, n) == 0
    assert lib.r3dgs_mip_opacity_backward(10, n, n, n, n, n, 0, n, 1.0, 1.0, 8, 8, 1.0, n, n, n, n, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_mip_filter3d(0, 3, n, n, n, n, n) == 0
    assert lib.r3dgs_mip_filter3d(10, -1, n, n, n, n, n) < 0 and "V out of range" in err()
    assert lib.r3dgs_mip_filter3d(10, 3, n, n, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_mip_filtered(0, n, n, n, n, n, n) == 0 and lib.r3dgs_mip_filtered_backward(0, n, n, n, n, n, n, n, n) == 0
    assert lib.r3dgs_mip_filtered(10, n, n, n, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_mip_filtered_backward(10, n, n, n, n, n, n, n, n) < 0 and "is NULL" in err()


def test_python_refusals_before_any_launch():
    import r3dgs_mip as mip
    rs = types.SimpleNamespace(viewmatrix=torch.eye(4), tanfovx=0.5, tanfovy=0.5, image_width=8, image_height=8, scale_modifier=1.0)
    m, o, s, q = torch.zeros(4, 3), torch.zeros(4, 1), torch.ones(4, 3), torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="antialias_opacity: means3D is a host tensor.*no CPU path"):
        mip.antialias_opacity(m, o, s, q, None, rs)
    with pytest.raises(TypeError, match="antialias_opacity: means3D is torch.float64"):
        mip.antialias_opacity(m.double(), o, s, q, None, rs)
    with pytest.raises(ValueError, match=r"antialias_opacity: means3D has shape \(4, 2\)"):
        mip.antialias_opacity(torch.zeros(4, 2), o, s, q, None, rs)
    with pytest.raises(RuntimeError, match="filtered_parameters: scaling_raw is a host tensor"):
        mip.filtered_parameters(s, o, torch.zeros(4, 1))
    with pytest.raises(ValueError, match=r"filtered_parameters: scaling_raw has shape \(4, 4\)"):
        mip.filtered_parameters(q, o, torch.zeros(4, 1))
    with pytest.raises(RuntimeError, match="filter_3d: xyz is a host tensor"):
        mip.filter_3d(m, torch.zeros(2, 20))
    with pytest.raises(TypeError, match="filter_3d: xyz must be a"):
        mip.filter_3d(None, torch.zeros(2, 20))
    cam = types.SimpleNamespace(world_view_transform=torch.eye(4), FoVx=2 * math.atan(0.5), FoVy=2 * math.atan(0.25),
                                image_width=100, image_height=50)
    table = mip.pack_cameras([cam, cam])
    assert table.shape == (2, 20) and table.dtype == torch.float32
    assert table[0, 16:].tolist() == pytest.approx([100.0, 100.0, 100.0, 50.0]) and torch.equal(table[0, :16], torch.eye(4).reshape(16))


# ---- render(): keywords, refusals, and the path with both keywords off ------------------------------------------------------

class _Pipe:
    debug = compute_cov3D_python = convert_SHs_python = False


def _fake_model(P=4):
    pc = types.SimpleNamespace(_xyz=torch.zeros(P, 3), _features_dc=torch.zeros(P, 1, 3), _features_rest=torch.zeros(P, 15, 3),
                               _opacity=torch.zeros(P, 1), _scaling=torch.zeros(P, 3), _rotation=torch.zeros(P, 4),
                               _degrees=torch.zeros(P, 1, dtype=torch.int32), active_sh_degree=3, max_sh_degree=3)
    pc.get_xyz = pc._xyz
    pc.get_covariance = lambda mod: torch.zeros(P, 6)
    return pc


def _fake_camera(grad=False):
    return types.SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4, requires_grad=grad),
                                 full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))


def test_render_signature_is_unchanged_and_both_off_is_todays_call(monkeypatch):
    import r3dgs_render
    sig = inspect.signature(r3dgs_render.render)
    assert list(sig.parameters) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color",
                                    "lambda_sh_sparsity", "measure_fps", "variable_sh_bands"]
    calls = []
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: calls.append((a, k)) or {"render": None})
    import r3dgs_mip
    launched = []
    monkeypatch.setattr(r3dgs_mip, "filtered_parameters", lambda *a: launched.append("filtered"))
    monkeypatch.setattr(r3dgs_mip, "antialias_opacity", lambda *a, **k: launched.append("antialias"))
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    r3dgs_render.render(cam, pc, _Pipe, bg)
    r3dgs_render.render(cam, pc, _Pipe, bg, antialiasing=False, filter_3d=None, scaling_modifier=0.5)
    assert calls == [((cam, pc, _Pipe, bg), {}), ((cam, pc, _Pipe, bg), {"scaling_modifier": 0.5})] and not launched
    assert calls[0][0][1] is pc, "the model itself, not a view of it"


def test_render_keywords_build_the_view_filter_first(monkeypatch):
    import r3dgs_mip
    import r3dgs_render
    seen, order = [], []
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: seen.append((a, k)) or {"render": None})
    s_eff, o_eff, o_aa = torch.ones(4, 3), torch.ones(4, 1), torch.full((4, 1), 2.0)

    def fake_filtered(scaling, opacity, f):
        order.append(("filtered", scaling, opacity, f))
        return s_eff, o_eff

    def fake_antialias(means3D, opacities, scales, rotations, cov, rs, raw=False):
        order.append(("antialias", means3D, opacities, scales, rotations, cov, rs, raw))
        return o_aa
    monkeypatch.setattr(r3dgs_mip, "filtered_parameters", fake_filtered)
    monkeypatch.setattr(r3dgs_mip, "antialias_opacity", fake_antialias)
    # the filter's own refusals (test_render_refusals) include "a host tensor", which is all this GPU-less test has: the
    # wiring is checked here with that one check taken out
    monkeypatch.setattr(r3dgs_render, "_checked_filter_3d", lambda f, pc: None)
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    f = torch.zeros(4, 1)
    r3dgs_render.render(cam, pc, _Pipe, bg, antialiasing=True, filter_3d=f, scaling_modifier=0.5)
    assert [o[0] for o in order] == ["filtered", "antialias"]
    assert order[0][1] is pc._scaling and order[0][2] is pc._opacity and order[0][3] is f
    _, means3D, opacities, scales, rotations, cov, rs, raw = order[1]
    assert means3D is pc._xyz and opacities is o_eff and scales is s_eff and rotations is pc._rotation and cov is None and raw is True
    assert rs.scale_modifier == 0.5 and rs.image_width == 8
    (a, k), = seen
    view = a[1]
    assert view is not pc and view._scaling is s_eff and view._opacity is o_aa and view._xyz is pc._xyz and view._rotation is pc._rotation
    assert view.active_sh_degree == 3 and torch.equal(view.get_scaling, torch.exp(s_eff)) and torch.equal(view.get_opacity, torch.sigmoid(o_aa))
    assert a[0] is cam and a[4] == 0.5 and r3dgs_render.fused_path_applies(view, _Pipe)
    # antialiasing alone with pipe.compute_cov3D_python: the compensation reads the model's own covariance
    order.clear()
    seen.clear()

    class CovPipe(_Pipe):
        compute_cov3D_python = True
    r3dgs_render.render(cam, pc, CovPipe, bg, antialiasing=True)
    assert [o[0] for o in order] == ["antialias"] and order[0][5] is not None and order[0][3] is None and order[0][7] is False
    assert seen[0][0][1]._scaling is pc._scaling


def test_render_refusals(monkeypatch):
    import r3dgs_mip
    import r3dgs_render
    from r3dgs_quantised import QuantisedModel
    launched = []
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: launched.append("render"))
    monkeypatch.setattr(r3dgs_mip, "filtered_parameters", lambda *a: launched.append("filtered"))
    monkeypatch.setattr(r3dgs_mip, "antialias_opacity", lambda *a, **k: launched.append("antialias"))
    monkeypatch.setattr(r3dgs_render, "_render_quantised", lambda *a, **k: launched.append("quantised"))
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    qm = object.__new__(QuantisedModel)
    for kw in ({"antialiasing": True}, {"filter_3d": torch.zeros(4, 1)}):
        with pytest.raises(ValueError, match="not available for a QuantisedModel"):
            r3dgs_render.render(cam, qm, _Pipe, bg, **kw)

    class CovPipe(_Pipe):
        compute_cov3D_python = True
    with pytest.raises(ValueError, match="filter_3d together with pipe.compute_cov3D_python"):
        r3dgs_render.render(cam, pc, CovPipe, bg, filter_3d=torch.zeros(4, 1))
    with pytest.raises(ValueError, match="antialiasing=True together with a camera that requires grad"):
        r3dgs_render.render(_fake_camera(grad=True), pc, _Pipe, bg, antialiasing=True)
    with pytest.raises(ValueError, match=r"filter_3d must be a \[P, 1\] tensor with P = 4.*got \(4,\)"):
        r3dgs_render.render(cam, pc, _Pipe, bg, filter_3d=torch.zeros(4))
    with pytest.raises(ValueError, match=r"filter_3d must be a \[P, 1\] tensor.*got \(5, 1\)"):
        r3dgs_render.render(cam, pc, _Pipe, bg, filter_3d=torch.zeros(5, 1))
    with pytest.raises(ValueError, match=r"filter_3d must be a \[P, 1\] tensor.*got list"):
        r3dgs_render.render(cam, pc, _Pipe, bg, filter_3d=[0.0] * 4)
    with pytest.raises(ValueError, match="filter_3d must be float32, got float64"):
        r3dgs_render.render(cam, pc, _Pipe, bg, filter_3d=torch.zeros(4, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="filter_3d must live on the model's device"):
        r3dgs_render.render(cam, pc, _Pipe, bg, filter_3d=torch.zeros(4, 1))   # a host tensor
    assert not launched, "a refused call launched something"
