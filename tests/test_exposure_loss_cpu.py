"""CPU-side checks of the exposure + mask loss (include/r3dgs_loss.h r3dgs_exposure_*, reduced-3dgs_amd/r3dgs_exposure.py,
csrc/exposure_math.h): the prototypes are exported and bound by both bindings, the workspace query, every refusal (none of
them launches anything, so they run without a GPU), the ExposureTable module, and the per-pixel map and adjoint of
exposure_math.h compiled for the host (tests/hostcheck_exposure) against float64.  No GPU needed."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import r3dgs_exposure
from diff_gaussian_rasterization import _C
from tests import exposure_loss_ref as ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_exposure", "hostcheck_exposure.hip")
SO = os.path.join(HERE, "hostcheck_exposure", "libhostcheck_exposure.so")
NAMES = ("r3dgs_exposure_loss_workspace_bytes", "r3dgs_exposure_loss_forward", "r3dgs_exposure_loss_backward",
         "r3dgs_exposure_apply")
F32 = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _last_error():
    return _C._lib.r3dgs_last_error().decode()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_prototypes_are_exported_and_bound_by_both_bindings():
    header = open(os.path.join(os.path.dirname(HERE), "include", "r3dgs_loss.h")).read()
    for name in NAMES:
        assert name + "(" in header, f"{name}: no prototype in include/r3dgs_loss.h"
        assert hasattr(_C._lib, name), f"{name}: not exported by the built library"
        assert name in _C._ABI["required"][1], f"{name}: no row in the required group"
        assert list(getattr(_C._lib, name).argtypes) == list(_C._ABI["required"][1][name][1])
    assert _C._OPTIONAL_ROWS["exposure"][1] == NAMES and _C.has_exposure_loss()
    assert _C._ext_loaded is not None, "the compiled binding is not built"
    assert set(NAMES) <= {n for n, _ in _C._ext_loaded.entry_points()}
    for fn in ("exposure_loss_forward", "exposure_loss_backward", "exposure_apply"):
        assert hasattr(_C._ext_loaded, fn) and hasattr(_C, fn)


def test_a_library_without_the_rows_says_so(monkeypatch):
    monkeypatch.setattr(_C, "_missing_rows", set(NAMES))
    assert not _C.has_exposure_loss()
    with pytest.raises(RuntimeError, match="no exposure loss entry points.*rebuild it with build.py"):
        _C.exposure_loss_workspace_bytes(1, 3, 8, 8)


def test_signatures():
    sig = inspect.signature(r3dgs_exposure.exposed_l1_dssim)
    assert list(sig.parameters) == ["image", "gt", "exposure", "mask", "mask_target", "lambda_dssim"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, 0.2]
    sig = inspect.signature(r3dgs_exposure.apply_exposure)
    assert list(sig.parameters) == ["image", "exposure", "clamp"] and sig.parameters["clamp"].default is False


def test_workspace_bytes():
    """The documented size: the forward's float slots [2][B*C*tiles], then the backward's double slots [12][B*tiles], with
    64 x 16 tiles; 0 for an invalid shape."""
    ws = _C._lib.r3dgs_exposure_loss_workspace_bytes
    for B, Cc, H, W in ((1, 3, 1, 1), (1, 3, 16, 64), (1, 3, 17, 65), (2, 3, 40, 70), (1, 3, 1062, 1600), (3, 1, 130, 23)):
        tiles = ((W + 63) // 64) * ((H + 15) // 16)
        assert ws(B, Cc, H, W) == 2 * B * Cc * tiles * 4 + 12 * B * tiles * 8, (B, Cc, H, W)
        assert ws(B, Cc, H, W) >= _C._lib.r3dgs_l1_ssim_workspace_bytes(B, Cc, H, W)
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (-1, 3, 8, 8), (1 << 20, 3, 1 << 14, 1 << 14)):
        assert ws(*bad) == 0, bad
    assert _C.exposure_loss_workspace_bytes(2, 3, 40, 70) == ws(2, 3, 40, 70)


# ---- refusals of the C calls: each returns < 0 with its message before anything is launched --------------------------------

def _call_forward(B=1, Cc=3, H=8, W=8, img1=1, img2=1, exposure=1, ws=1, ws_bytes=None):
    """Non-NULL arguments are HOST buffers: the calls under test must refuse before they launch, so nothing reads them."""
    n = max(B * Cc * H * W, 1) if min(B, Cc, H, W) > 0 and B * Cc * H * W < 1 << 20 else 1
    buf = np.zeros(n, F32)
    e = np.zeros(12 * max(B, 1) if B < 1 << 10 else 12, F32)
    need = _C._lib.r3dgs_exposure_loss_workspace_bytes(B, Cc, H, W)
    w = np.zeros(max(need, 8), np.uint8)
    return _C._lib.r3dgs_exposure_loss_forward(B, Cc, H, W, _p(buf) if img1 else None, _p(buf) if img2 else None,
                                               _p(e) if exposure else None, 1, None, 0, 0, 0.2, None, None, None, None, None,
                                               None, _p(w) if ws else None, need if ws_bytes is None else ws_bytes, None)


def _call_backward(B=1, Cc=3, H=8, W=8, exposure=1, partials=1, grad=1, dx=1, dE=0, ws=1, ws_bytes=None):
    n = max(B * Cc * H * W, 1) if min(B, Cc, H, W) > 0 and B * Cc * H * W < 1 << 20 else 1
    buf, part, e = np.zeros(n, F32), np.zeros(3 * n, F32), np.zeros(12 * max(B, 1), F32)
    need = _C._lib.r3dgs_exposure_loss_workspace_bytes(B, Cc, H, W)
    w = np.zeros(max(need, 8), np.uint8)
    return _C._lib.r3dgs_exposure_loss_backward(B, Cc, H, W, _p(buf), _p(buf), _p(e) if exposure else None, 1, None, 0, 0,
                                                _p(part) if partials else None, _p(buf) if grad else None, 0.8, -0.2,
                                                _p(buf) if dx else None, _p(e) if dE else None, _p(w) if ws else None,
                                                need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("call", [_call_forward, _call_backward], ids=["forward", "backward"])
def test_c_calls_refuse(call):
    what = "exposure_loss_" + ("forward" if call is _call_forward else "backward")
    for shape in ((0, 3, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (1, 0, 8, 8)):
        assert call(*shape) < 0
        assert _last_error().startswith(what + ": need B, C, H, W >= 1"), _last_error()
    for Cc in (1, 2, 4):
        assert call(1, Cc, 8, 8) < 0
        assert _last_error() == f"{what}: an exposure maps 3 colour channels, the images have C = {Cc}"
    assert call(ws=0) < 0 and _last_error() == what + ": a required pointer is NULL"
    need = _C._lib.r3dgs_exposure_loss_workspace_bytes(1, 3, 8, 8)
    for short in (0, need - 1, _C._lib.r3dgs_l1_ssim_workspace_bytes(1, 3, 8, 8)):
        assert call(ws_bytes=short) < 0
        assert _last_error() == f"{what}: the workspace holds {short} bytes, this shape needs {need} (r3dgs_exposure_loss_workspace_bytes)"


def test_c_calls_refuse_null_pointers():
    assert _call_forward(img1=0) < 0 and _last_error() == "exposure_loss_forward: a required pointer is NULL"
    assert _call_forward(img2=0) < 0 and _last_error() == "exposure_loss_forward: a required pointer is NULL"
    for missing in ("partials", "grad", "dx"):
        assert _call_backward(**{missing: 0}) < 0
        assert _last_error() == "exposure_loss_backward: a required pointer is NULL", missing
    assert _call_backward(exposure=0, dE=1) < 0
    assert _last_error() == "exposure_loss_backward: grad_exposure is asked for without an exposure"


def test_c_calls_refuse_a_misaligned_workspace():
    """The workspace holds double sums: a buffer that is not 8-byte aligned is refused, not written with misaligned stores."""
    buf, part, e = np.zeros(3 * 64, F32), np.zeros(9 * 64, F32), np.zeros(12, F32)
    need = _C._lib.r3dgs_exposure_loss_workspace_bytes(1, 3, 8, 8)
    w = np.zeros(need + 16, np.uint8)
    base = w.ctypes.data + (-w.ctypes.data) % 8
    for off in (1, 4):
        ws = C.c_void_p(base + off)
        assert _C._lib.r3dgs_exposure_loss_forward(1, 3, 8, 8, _p(buf), _p(buf), _p(e), 0, None, 0, 0, 0.2, None, None, None, None,
                                                   None, None, ws, need, None) < 0
        assert _last_error() == "exposure_loss_forward: the workspace must be 8-byte aligned (it holds double sums)"
        assert _C._lib.r3dgs_exposure_loss_backward(1, 3, 8, 8, _p(buf), _p(buf), _p(e), 0, None, 0, 0, _p(part), _p(buf), 0.8, -0.2,
                                                    _p(buf), _p(e), ws, need, None) < 0
        assert _last_error() == "exposure_loss_backward: the workspace must be 8-byte aligned (it holds double sums)"


def test_exposure_apply_refuses():
    buf, e = np.zeros(3 * 64, F32), np.zeros(12, F32)
    apply = _C._lib.r3dgs_exposure_apply
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -2)):
        assert apply(B, H, W, _p(buf), _p(e), 0, 0, _p(buf), None) < 0
        assert _last_error().startswith("exposure_apply: need B, H, W >= 1")
    for args in ((None, _p(e), _p(buf)), (_p(buf), None, _p(buf)), (_p(buf), _p(e), None)):
        assert apply(1, 8, 8, args[0], args[1], 0, 0, args[2], None) < 0
        assert _last_error() == "exposure_apply: a required pointer is NULL"


# ---- refusals of the Python layer ---------------------------------------------------------------------------------------------

def test_python_layer_refuses():
    f = r3dgs_exposure.exposed_l1_dssim
    a, b = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    E, m = torch.eye(3, 4), torch.ones(16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(a, b, E, m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_exposure.apply_exposure(a, E)
    with pytest.raises(TypeError, match="float32"):
        f(a.half(), b.half(), E, m)
    with pytest.raises(TypeError, match="exposure is torch.float64"):
        f(a, b, E.double(), m)
    with pytest.raises(TypeError, match="mask is torch.bool"):
        f(a, b, E, m.bool())
    with pytest.raises(TypeError, match="float32"):
        r3dgs_exposure.apply_exposure(a.double(), E)
    with pytest.raises(RuntimeError, match="target requires grad"):
        f(a, b.clone().requires_grad_(), E, m)
    with pytest.raises(RuntimeError, match="mask requires grad"):
        f(a, b, E, m.clone().requires_grad_())
    with pytest.raises(ValueError, match="3 colour channels"):
        f(torch.rand(4, 16, 16), torch.rand(4, 16, 16), E)
    with pytest.raises(ValueError, match=r"exposure of shape \(3, 4\) or \(1, 3, 4\)"):
        f(a, b, torch.eye(4, 4))
    with pytest.raises(ValueError, match=r"exposure of shape \(3, 4\) or \(2, 3, 4\)"):
        f(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16), torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="expected a mask of shape"):
        f(a, b, E, torch.ones(16, 15))
    with pytest.raises(ValueError, match="expected a mask of shape"):
        f(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16), None, torch.ones(2, 16, 16))
    with pytest.raises(ValueError, match="shapes differ"):
        f(a, torch.rand(3, 16, 17), E, m)
    with pytest.raises(TypeError, match="must be a tensor"):
        f(a, b, np.eye(3, 4, dtype=F32))


# ---- ExposureTable ------------------------------------------------------------------------------------------------------------

def test_exposure_table():
    t = r3dgs_exposure.ExposureTable(5)
    assert len(t) == 5 and [tuple(p.shape) for p in t.parameters()] == [(5, 3, 4)]
    assert t.exposure.dtype == torch.float32 and t.exposure.requires_grad
    assert torch.equal(t.exposure.detach(), torch.eye(3, 4).expand(5, 3, 4))
    assert t[2].shape == (3, 4) and t[2].requires_grad and t[torch.tensor([0, 3])].shape == (2, 3, 4)
    assert t[2].data_ptr() == t.exposure[2].data_ptr(), "table[idx] is a view of the parameter"
    with torch.no_grad():
        t.exposure.add_(torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(0)))
    other = r3dgs_exposure.ExposureTable(5)
    assert list(t.state_dict()) == ["exposure"]
    other.load_state_dict(t.state_dict())
    assert torch.equal(other.exposure, t.exposure)
    (t[1] * 2.0).sum().backward()   # the gradient reaches the used row alone
    assert torch.equal(t.exposure.grad[1], torch.full((3, 4), 2.0)) and not t.exposure.grad[[0, 2, 3, 4]].any()
    torch.optim.Adam(t.parameters(), lr=1e-2).step()
    with pytest.raises(ValueError):
        r3dgs_exposure.ExposureTable(0)


# ---- exposure_math.h on the host ------------------------------------------------------------------------------------------------

def _shim():
    return build_shim(SRC, SO, EXACT, "hipcc not available to build the exposure host-check shim")


def _random_pixels(n, seed):
    rng = np.random.default_rng(seed)
    E = (np.tile(np.eye(3, 4), (n, 1, 1)) + rng.normal(0, 0.3, (n, 3, 4))).astype(F32)
    x = rng.uniform(-0.5, 2.0, (n, 3)).astype(F32)
    g = rng.normal(0, 1, (n, 3)).astype(F32)
    m = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.2, 1.0, n)).astype(F32)
    return E, x, g, m


def _map64(E, x, m):
    E, x, m = E.astype(np.float64), x.astype(np.float64), m.astype(np.float64)
    return m[:, None] * (np.einsum("nk,nkc->nc", x, E[:, :, :3]) + E[:, :, 3])


def _adjoint64(E, g, m):
    E, g, m = E.astype(np.float64), g.astype(np.float64), m.astype(np.float64)
    return m[:, None] * np.einsum("nkc,nc->nk", E[:, :, :3], g)


def _run(lib, E, x, g, m):
    n = len(m)
    out, dx, dE = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 3, 4), np.float64)
    lib.hc_exposed(n, _p(E), _p(x), _p(m), _p(out))
    lib.hc_exposed_adjoint(n, _p(E), _p(g), _p(m), _p(dx))
    lib.hc_exposure_grad_terms(n, _p(x), _p(g), _p(m), _p(dE))
    return out, dx, dE


def test_host_map_and_adjoint_match_float64():
    """The issue asks for "1e-6 relative".  Read here, on purpose, as 1e-6 of the sum of the magnitudes of a value's terms: the
    map and the adjoint are sums of up to four signed products that can cancel, and the rounding of such a sum scales with its
    terms, not with what is left of them (relative to the result alone the bar would be unbounded at a cancellation, for any
    fp32 evaluation).  Where nothing cancels the two readings coincide.  The dE terms are single products: plain 1e-6 relative."""
    lib = _shim()
    n = 20000
    E, x, g, m = _random_pixels(n, 5)
    out, dx, dE = _run(lib, E, x, g, m)
    a = np.abs
    scale = m[:, None] * (np.einsum("nk,nkc->nc", a(x), a(E[:, :, :3])) + a(E[:, :, 3]))
    assert (a(out - _map64(E, x, m)) <= 1e-6 * scale).all()
    scale = m[:, None] * np.einsum("nkc,nc->nk", a(E[:, :, :3]), a(g))
    assert (a(dx - _adjoint64(E, g, m)) <= 1e-6 * scale).all()
    mg = m.astype(np.float64)[:, None] * g.astype(np.float64)
    want = np.concatenate([x.astype(np.float64)[:, :, None] * mg[:, None, :], mg[:, :, None]], axis=2)   # [n,3,4]: dE[k][c], dE[c][3]
    assert (a(dE - want) <= 1e-6 * a(want)).all()


def test_host_identity_is_bit_exact():
    """E = eye(3,4), m = 1: x'' == x and dx == g bit for bit, zeros of either sign and denormals included."""
    lib = _shim()
    n = 20000
    _, x, g, _ = _random_pixels(n, 6)
    special = np.array([0.0, -0.0, 1e-42, -1e-42, 3.0e38, -3.0e38, 1.0, -1.0], F32)
    x[:len(special), 0], x[:len(special), 1], x[:len(special), 2] = special, special[::-1], -special
    g[:len(special)] = x[:len(special)]
    E = np.tile(np.eye(3, 4, dtype=F32), (n, 1, 1))
    out, dx, _ = _run(lib, E, x, g, np.ones(n, F32))
    assert np.array_equal(out.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(dx.view(np.uint32), g.view(np.uint32))


def test_host_adjoint_is_the_transpose_of_the_map():
    """<g, J v> == <J^T g, v> to 1e-6 of the sum of the magnitudes of the terms: J v is the map without its offset (the
    exposure's last column zeroed), J^T g the adjoint; and <dE terms, dE direction> is the map's derivative along E."""
    lib = _shim()
    n = 20000
    E, v, g, m = _random_pixels(n, 7)
    E0 = E.copy()
    E0[:, :, 3] = 0
    Jv, JTg, dE = _run(lib, E0, v, g, m)
    lhs = (g.astype(np.float64) * Jv).sum(1)
    rhs = (JTg.astype(np.float64) * v).sum(1)
    a = np.abs
    scale = m * np.einsum("nk,nkc,nc->n", a(v), a(E[:, :, :3]), a(g)).astype(np.float64)
    assert (a(lhs - rhs) <= 1e-6 * scale).all() and (scale[m > 0] > 0).all()
    # along a direction D of the exposure the map moves by m (v D[:, :3] + D[:, 3]): <g, that> == <dE terms, D>
    D = np.random.default_rng(8).normal(0, 1, (n, 3, 4))
    moved = m[:, None].astype(np.float64) * (np.einsum("nk,nkc->nc", v.astype(np.float64), D[:, :, :3]) + D[:, :, 3])
    lhs, rhs = (g.astype(np.float64) * moved).sum(1), (dE * D).sum((1, 2))
    scale = m * (np.einsum("nk,nkc,nc->n", a(v), a(D[:, :, :3]), a(g)) + np.einsum("nc,nc->n", a(D[:, :, 3]), a(g)))
    assert (a(lhs - rhs) <= 1e-6 * scale).all()


# ---- the test inputs' own properties (tests/exposure_loss_ref.py), checked against the float64 reference --------------------

@pytest.mark.parametrize("mask_target", [False, True])
def test_inputs_keep_every_exposure_gradient_entry_large(mask_target):
    """The recipe of exposure_loss_ref.inputs keeps dE from being the remainder of a cancellation: the smallest entry is at
    least 5 % of the largest, so a bar relative to the tensor's maximum masks nothing out."""
    x, y, m = ref.inputs((3, 40, 70), seed=11)
    E = ref.exposure_guess(1, seed=12)[0]
    r = ref.evaluate(x, y, E, m, mask_target)
    assert np.abs(r["dE"]).min() >= 0.05 * np.abs(r["dE"]).max()
    assert abs((m == 0).mean() - 0.3) < 0.05 and m[m > 0].min() >= 0.2
