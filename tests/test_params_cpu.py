"""CPU checks of the raw-parameter path (csrc/param_math.h, include/r3dgs_rasterizer.h r3dgs_*_params,
diff_gaussian_rasterization.rasterize_gaussian_params, r3dgs_render.render).  The activation arithmetic the kernels execute
per lane runs on the host through tests/hostcheck_params and is held to float64 -- F.normalize within 2 ulp, the backward
within the bounds param_math.h derives from its own rounding count -- with torch's float64 autograd as a second witness;
the four new symbols are declared, exported and bound twice; what the path does not cover is refused with a message.
No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from tests.hostcheck_build import EXACT, build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_params", "hostcheck_params.hip")
SO = os.path.join(HERE, "hostcheck_params", "libhostcheck_params.so")
HDR = os.path.join(ROOT, "reduced-3dgs_amd", "csrc", "param_math.h")
F32 = np.float32
REF = "/root/reference"   # as tests/test_reference_imports.py: only present where the suite is authored
NEW = ("r3dgs_forward_params", "r3dgs_forward_params_reserved", "r3dgs_backward_params", "r3dgs_activate_params")


def shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the parameter host-check shim")
    lib.hc_normalize_eps.restype = C.c_float
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_quat_act(lib, raw):
    raw = np.ascontiguousarray(raw, F32)
    q, n = np.empty_like(raw), np.empty(len(raw), F32)
    lib.hc_quat_act(len(raw), _p(raw), _p(q), _p(n))
    return q, n


def host_quat_act_bwd(lib, q, n, g):
    q, n, g = (np.ascontiguousarray(x, F32) for x in (q, n, g))
    out = np.empty_like(q)
    lib.hc_quat_act_bwd(len(q), _p(q), _p(n), _p(g), _p(out))
    return out


def host_scale_act(lib, raw):
    raw = np.ascontiguousarray(raw, F32)
    s = np.empty_like(raw)
    lib.hc_scale_act(raw.size, _p(raw), _p(s))
    return s


def host_scale_act_bwd(lib, g, s):
    g, s = np.ascontiguousarray(g, F32), np.ascontiguousarray(s, F32)
    out = np.empty_like(g)
    lib.hc_scale_act_bwd(g.size, _p(g), _p(s), _p(out))
    return out


def quaternions(rng, n=4000):
    """Random quaternions over 40 decades of norm, plus the cases the issue names."""
    raw = rng.standard_normal((n, 4)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    unit = rng.standard_normal((5, 4))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    special = [np.zeros(4), unit[0] * 1e-20, unit[1] * 1e15, unit[2] * 1e-12, unit[3] * 3e-13, unit[4],
               np.array([1.0, 0, 0, 0]), np.array([0, 0, 0, -2.5]), np.array([1e-30, 0, 0, 0]), np.array([3.0, 4.0, 0, 0])]
    return np.concatenate([np.array(special), raw]).astype(F32)


def ulp(x):
    return np.spacing(np.abs(x).astype(F32)).astype(np.float64)


def test_normalize_forward_within_2_ulp_of_float64():
    lib = shim()
    rng = np.random.default_rng(1)
    raw = quaternions(rng)
    q, n = host_quat_act(lib, raw)
    r64 = raw.astype(np.float64)
    n64 = np.sqrt((r64 * r64).sum(1))
    ref = r64 / np.maximum(n64, 1e-12)[:, None]
    tref = F.normalize(torch.from_numpy(r64), dim=1).numpy()     # second witness
    assert np.allclose(ref, tref, rtol=1e-14, atol=0)
    err = np.abs(q.astype(np.float64) - ref) / ulp(ref.astype(F32))
    print("normalize: max error", err.max(), "ulp")
    assert err.max() <= 2.0
    assert np.abs(n.astype(np.float64) - n64).max() <= 0 or (np.abs(n.astype(np.float64) - n64) / np.maximum(ulp(n64.astype(F32)), 1e-300)).max() <= 0.5 + 1e-6
    assert not np.isnan(q).any() and np.array_equal(q[0], np.zeros(4, F32))   # the zero quaternion stays zero
    assert abs(lib.hc_normalize_eps() - 1e-12) <= 1e-12 * 2.0 ** -24


def test_quat_backward_within_the_headers_bound():
    lib = shim()
    rng = np.random.default_rng(2)
    raw = quaternions(rng)
    g = (rng.standard_normal(raw.shape) * 10.0 ** rng.uniform(-6, 3, (len(raw), 1))).astype(F32)
    q, n = host_quat_act(lib, raw)
    got = host_quat_act_bwd(lib, q, n, g).astype(np.float64)
    # float64 from the same fp32 raw and g, branch by the exact norm as the issue states it
    r64, g64 = raw.astype(np.float64), g.astype(np.float64)
    n64 = np.sqrt((r64 * r64).sum(1))
    q64 = r64 / np.maximum(n64, 1e-12)[:, None]
    ref = np.where((n64 > 1e-12)[:, None], (g64 - q64 * (q64 * g64).sum(1, keepdims=True)) / np.maximum(n64, 1e-300)[:, None],
                   g64 / 1e-12)
    bound = np.empty_like(ref)
    lib.hc_quat_act_bwd_bound(len(raw), _p(np.ascontiguousarray(q64)), _p(np.ascontiguousarray(n64)), _p(np.ascontiguousarray(g64)),
                              _p(bound))
    # a norm within one fp32 rounding of the clamp may take the other branch in fp32: the issue fixes the branch by n
    near = np.abs(n64 - 1e-12) <= 1e-12 * 2.0 ** -22
    err = np.abs(got - ref)
    ok = near | (err <= bound).all(1)
    print("quat backward: max err / bound", (err[~near] / np.maximum(bound[~near], 1e-300)).max())
    assert ok.all(), (raw[~ok][:3], err[~ok][:3], bound[~ok][:3])
    # second witness: torch's float64 autograd of F.normalize (its clamp passes the gradient at n >= eps)
    t = torch.from_numpy(r64).requires_grad_()
    (F.normalize(t, dim=1) * torch.from_numpy(g64)).sum().backward()
    terr = np.abs(got - t.grad.numpy())
    assert (near | (terr <= bound + 1e-12 * np.abs(t.grad.numpy())).all(1)).all()
    assert np.isfinite(got).all()


def test_scale_backward_within_the_headers_bound():
    lib = shim()
    rng = np.random.default_rng(3)
    raw = np.concatenate([np.array([-20.0, 20.0, 0.0, -1e-3, 5.0, -87.0, 88.0]), rng.uniform(-20, 20, 4000)]).astype(F32)
    g = (rng.standard_normal(raw.shape) * 10.0 ** rng.uniform(-6, 3, raw.shape)).astype(F32)
    s = host_scale_act(lib, raw)
    ref_s = np.exp(raw.astype(np.float64))
    exp_ulps = (np.abs(s.astype(np.float64) - ref_s) / ulp(ref_s.astype(F32))).max()
    print("host expf: max error", exp_ulps, "ulp")
    assert exp_ulps <= 1.0    # what the bound's c = 1 + 2 * exp_ulps is evaluated with below
    got = host_scale_act_bwd(lib, g, s).astype(np.float64)
    # against the exact product of its own fp32 inputs: c = 1
    exact = g.astype(np.float64) * s.astype(np.float64)
    b0 = np.empty_like(exact)
    lib.hc_scale_act_bwd_bound(len(g), _p(g.astype(np.float64)), _p(s.astype(np.float64)), C.c_double(0.0), _p(b0))
    assert (np.abs(got - exact) <= b0).all()
    assert np.array_equal(got.astype(F32), (g * s).astype(F32))   # one IEEE product
    # against float64 of the raw value, torch's autograd of exp as the witness: c = 1 + 2 * exp_ulps
    t = torch.from_numpy(raw.astype(np.float64)).requires_grad_()
    (torch.exp(t) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    b1 = np.empty_like(exact)
    lib.hc_scale_act_bwd_bound(len(g), _p(g.astype(np.float64)), _p(ref_s), C.c_double(1.0), _p(b1))
    err = np.abs(got - t.grad.numpy())
    print("scale backward: max err / bound", (err / np.maximum(b1, 1e-300)).max())
    assert (err <= b1).all()


def test_header_documents_its_rounding_counts():
    src = open(HDR).read()
    for word in ("((x0 * x0 + x1 * x1) + x2 * x2) + x3 * x3", "((q[0] * g[0] + q[1] * g[1]) + q[2] * g[2]) + q[3] * g[3]",
                 "quat_act_bwd_bound", "scale_act_bwd_bound", "kUnitRoundoff"):
        assert word in src, word


# ---- the boundary -----------------------------------------------------------------------------------------------------

def test_new_symbols_declared_exported_and_bound_twice():
    hdr = open(os.path.join(ROOT, "include", "r3dgs_rasterizer.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from diff_gaussian_rasterization import _C
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} not declared"
        assert hasattr(_C._lib, name), f"{name} not exported"
        assert getattr(_C._lib, name).argtypes is not None, f"{name} has no ctypes prototype"
        assert (name, False) in _C._ext_loaded.entry_points(), f"{name} is not handed to the compiled binding"
    # the signatures the issue derives from the existing ones
    sig = re.search(r"r3dgs_backward_params\s*\((.*?)\);", code, flags=re.S).group(1)
    for word in ("features_dc", "features_rest", "scaling_raw", "rotation_raw", "dL_dfeatures_dc", "dL_dfeatures_rest",
                 "dL_dscaling_raw", "dL_drotation_raw"):
        assert word in sig
    assert "colors_precomp" not in sig and "cov3D_precomp" not in sig
    assert _C._ext_loaded is not None, "the compiled binding is not built"
    for name in ("forward_params", "forward_params_reserved", "backward_params", "activate_params"):
        assert callable(getattr(_C._ext_loaded, name))
    for name in ("rasterize_gaussian_params", "rasterize_gaussian_params_backward", "activate_params"):
        assert callable(getattr(_C, name))
    # the existing surface is as it was
    import diff_gaussian_rasterization as dgr
    assert list(inspect.signature(dgr.rasterize_gaussian_params).parameters) == [
        "xyz", "means2D", "features_dc", "features_rest", "degrees", "opacity", "scaling", "rotation", "raster_settings",
        "lambda_sh_sparsity"]


def _cpu_args(P=4, M=16, **over):
    a = dict(background=torch.zeros(3), xyz=torch.zeros(P, 3), features_dc=torch.zeros(P, 1, 3),
             features_rest=torch.zeros(P, M - 1, 3), degrees=torch.zeros(P, dtype=torch.int32), opacity=torch.zeros(P, 1),
             scaling=torch.zeros(P, 3), rotation=torch.zeros(P, 4))
    a.update(over)
    return tuple(a.values()) + (1.0, torch.eye(4), torch.eye(4), 1.0, 1.0, 16, 16, torch.zeros(3), False, False)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_refusals(binding):
    from diff_gaussian_rasterization import _C
    was = _C.set_binding(binding)
    try:
        with pytest.raises(RuntimeError, match="no CPU path"):
            _C.rasterize_gaussian_params(*_cpu_args())
        with pytest.raises(RuntimeError, match="no CPU path"):
            _C.activate_params(torch.zeros(4, 3), torch.zeros(4, 4))
        with pytest.raises(RuntimeError, match=r"means3D must have dimensions"):
            _C.rasterize_gaussian_params(*_cpu_args(xyz=torch.zeros(4, 4)))
    finally:
        _C.set_binding(was)
    # shape / dtype / layout refusals are decided before anything touches a device: exercise the checker itself, on
    # meta tensors that claim to live on the GPU (no GPU is needed to construct them)
    dev = torch.device("cuda", 0)

    def m(*shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device="meta")
        return t

    class OnDev:   # a tensor-like that reports device cuda:0 and forwards the rest to a meta tensor
        def __init__(self, t):
            self._t = t
            self.device = dev

        def __getattr__(self, k):
            return getattr(self._t, k)

    def args(P=4, M=16, **over):
        a = dict(xyz=OnDev(m(P, 3)), features_dc=OnDev(m(P, 1, 3)), features_rest=OnDev(m(P, M - 1, 3)),
                 opacity=OnDev(m(P, 1)), scaling=OnDev(m(P, 3)), rotation=OnDev(m(P, 4)),
                 degrees=OnDev(m(P, dtype=torch.int32)))
        a.update(over)
        return a
    assert _C._check_params(**args())[:2] == (4, 16)
    assert _C._check_params(**args(features_rest=None))[:2] == (4, 1)
    with pytest.raises(RuntimeError, match=r"features_rest must have dimensions \(num_points, M-1, 3\)"):
        _C._check_params(**args(features_rest=OnDev(m(4, 45))))
    with pytest.raises(RuntimeError, match=r"features_rest must have dimensions \(num_points, M-1, 3\)"):
        _C._check_params(**args(features_rest=OnDev(m(5, 15, 3))))
    with pytest.raises(RuntimeError, match=r"M <= 16"):
        _C._check_params(**args(features_rest=OnDev(m(4, 16, 3))))
    with pytest.raises(RuntimeError, match=r"features_dc must have dimensions"):
        _C._check_params(**args(features_dc=OnDev(m(4, 3))))
    with pytest.raises(RuntimeError, match="needs float32"):
        _C._check_params(**args(scaling=OnDev(m(4, 3, dtype=torch.float64))))
    with pytest.raises(RuntimeError, match="needs float32"):
        _C._check_params(**args(features_rest=OnDev(m(4, 15, 3, dtype=torch.float16))))
    with pytest.raises(RuntimeError, match="needs a contiguous tensor"):
        _C._check_params(**args(rotation=OnDev(m(4, 8)[:, ::2])))
    with pytest.raises(RuntimeError, match="needs a contiguous tensor"):
        _C._check_params(**args(features_rest=OnDev(m(4, 3, 15).transpose(1, 2))))


def test_c_abi_refusals():
    """The C entry points refuse a features_rest that does not match M before anything is launched."""
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    one = C.c_void_p(256)   # never dereferenced: the checks come first
    st = lib.r3dgs_forward_params_reserved(one, one, one, 1, 4, one, 16, one, 16, 16, one, one, None, one, one, 1.0, one, one,
                                           one, one, 1.0, 1.0, 0, one, None, None, None, 0, 0, None)
    assert st < 0 and b"features_rest must be [P,M-1,3]" in lib.r3dgs_last_error()
    st = lib.r3dgs_forward_params_reserved(one, one, one, 1, 4, one, 1, one, 16, 16, one, one, one, one, one, 1.0, one, one,
                                           one, one, 1.0, 1.0, 0, one, None, None, None, 0, 0, None)
    assert st < 0 and b"features_rest must be [P,M-1,3]" in lib.r3dgs_last_error()
    st = lib.r3dgs_forward_params_reserved(one, one, one, 1, 4, one, 17, one, 16, 16, one, one, one, one, one, 1.0, one, one,
                                           one, one, 1.0, 1.0, 0, one, None, None, None, 0, 0, None)
    assert st < 0 and b"[1,16]" in lib.r3dgs_last_error()
    st = lib.r3dgs_activate_params(4, one, None, None, None, None)
    assert st < 0 and b"activate_params" in lib.r3dgs_last_error()


# ---- r3dgs_render ------------------------------------------------------------------------------------------------------

def test_render_surface():
    import r3dgs_render
    sig = inspect.signature(r3dgs_render.render)
    assert list(sig.parameters) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color",
                                    "lambda_sh_sparsity", "measure_fps", "variable_sh_bands"]
    assert sig.parameters["scaling_modifier"].default == 1.0 and sig.parameters["override_color"].default is None
    assert sig.parameters["lambda_sh_sparsity"].default == 0.
    src = inspect.getsource(r3dgs_render.render)
    for key in ("render", "viewspace_points", "visibility_filter", "radii", "FPS"):
        assert f'"{key}"' in src

    class Pipe:
        debug = compute_cov3D_python = convert_SHs_python = False

    class PC:
        _xyz, _features_dc, _features_rest = torch.zeros(4, 3), torch.zeros(4, 1, 3), torch.zeros(4, 15, 3)
        _opacity, _scaling, _rotation = torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 4)
    assert r3dgs_render.fused_path_applies(PC, Pipe)
    assert not r3dgs_render.fused_path_applies(PC, Pipe, override_color=torch.zeros(4, 3))
    assert not r3dgs_render.fused_path_applies(PC, Pipe, variable_sh_bands=True)
    Pipe.convert_SHs_python = True
    assert not r3dgs_render.fused_path_applies(PC, Pipe)
    Pipe.convert_SHs_python, Pipe.compute_cov3D_python = False, True
    assert not r3dgs_render.fused_path_applies(PC, Pipe)


def test_render_matches_the_reference_signature():
    """Keyword names, defaults and result keys of the reference's gaussian_renderer.render, read from its source (the
    module itself imports the CUDA extension and cannot be imported here)."""
    import ast
    ref = os.path.join(REF, "gaussian_renderer", "__init__.py")
    if not os.path.exists(ref):
        pytest.skip("reference checkout not present")
    import r3dgs_render
    fn = next(n for n in ast.parse(open(ref).read()).body if isinstance(n, ast.FunctionDef) and n.name == "render")
    names = [a.arg for a in fn.args.args]
    assert list(inspect.signature(r3dgs_render.render).parameters) == names
    defaults = [ast.literal_eval(d) for d in fn.args.defaults]
    mine = [p.default for p in inspect.signature(r3dgs_render.render).parameters.values() if p.default is not inspect._empty]
    assert mine == defaults
    ret = next(n for n in ast.walk(fn) if isinstance(n, ast.Return))
    keys = [ast.literal_eval(k) for k in ret.value.keys]
    src = inspect.getsource(r3dgs_render.render)
    for k in keys:
        assert f'"{k}"' in src
