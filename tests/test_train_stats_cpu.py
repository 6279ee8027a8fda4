"""CPU checks of the per-iteration training statistics (reduced-3dgs_amd/r3dgs_train_stats.py, csrc/train_stats.hip,
include/r3dgs_trainstats.h): the per-element kernel arithmetic (csrc/stats_math.h) runs on the host through a test shim; the
accumulator update must equal the numpy restatement (tests/trainstats_ref.py) bit for bit, the sigmoid and its derivative stay
within the bound derived there from the documented accuracy of expf; the Python surface refuses what the kernels do not take.
No GPU needed."""
import ctypes as C
import inspect
import os
import re
import zlib

import numpy as np
import pytest
import torch

import r3dgs_train_stats as ts
from tests import trainstats_ref as ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck_stats", "hostcheck_stats.hip")
SO = os.path.join(HERE, "hostcheck_stats", "libhostcheck_stats.so")
F32 = np.float32


def _shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the statistics host-check shim")
    lib.hc_alpha_regul_term.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def _gradients(rng, n, kind):
    mag = 10.0 ** rng.uniform(-8, 3, (n, 3))
    vg = (rng.standard_normal((n, 3)) * mag).astype(F32)
    if kind == "zeros":
        vg[::3, 0] = 0
        vg[1::3, 1] = 0
        vg[::5] = 0
    elif kind == "denormals":   # below 2^-126: the squares underflow to zero, sums of denormal squares stay exact or flush
        vg = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-45, -37, (n, 3))).astype(F32)
        vg[::4, 0] = (rng.standard_normal(len(vg[::4])) * 1e-20).astype(F32)   # a denormal square next to a normal one
    return vg


@pytest.mark.parametrize("kind", ["random", "zeros", "denormals"])
@pytest.mark.parametrize("start", ["zero", "nonzero"])
def test_accumulator_update_on_host_matches_the_restatement_bit_for_bit(kind, start):
    """densify_update (csrc/stats_math.h) on the CPU == tests/trainstats_ref.densification_stats, all three accumulators, with
    radii among 0, 1 and 2^20 and gradient rows that are non-zero under culled Gaussians too."""
    lib = _shim()
    n = 20_000
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{start}".encode()))
    vg = _gradients(rng, n, kind)
    radii = rng.choice(np.array([0, 1, 1 << 20], np.int32), n).astype(np.int32)
    if start == "zero":
        acc, den, mx = np.zeros((n, 1), F32), np.zeros((n, 1), F32), np.zeros(n, F32)
    else:
        acc = (10.0 ** rng.uniform(-6, 2, (n, 1))).astype(F32)
        den = rng.integers(0, 3000, (n, 1)).astype(F32)
        mx = rng.choice(np.array([0.0, 0.5, 1.0, 37.0, 2.0 ** 20, 2.0 ** 21], F32), n).astype(F32)
    want = ref.densification_stats(vg, radii, acc, den, mx)
    got = [np.array(a, F32) for a in (acc, den, mx)]
    lib.hc_densification_stats(n, _p(vg), _p(radii), *(_p(a) for a in got))
    for name, a, b in zip(("xyz_gradient_accum", "denom", "max_radii2D"), got, want):
        assert _bits_equal(a, b), f"{name}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements differ"
    culled = radii == 0
    assert culled.any() and np.abs(vg[culled, :2]).max() > 0
    for a, b in zip(got, (acc, den, mx)):   # a culled Gaussian changes nothing, whatever its gradient row holds
        assert _bits_equal(a.reshape(-1)[culled], b.reshape(-1)[culled])


def _sigmoid_inputs():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-ref.SIGMOID_DOMAIN, ref.SIGMOID_DOMAIN, 200_000), rng.standard_normal(200_000) * 4,
                        rng.standard_normal(50_000) * 1e-3,
                        np.array([0.0, -0.0, 1e-30, -1e-30, ref.SIGMOID_DOMAIN, -ref.SIGMOID_DOMAIN, -2.1972246])])
    return np.ascontiguousarray(np.clip(x, -ref.SIGMOID_DOMAIN, ref.SIGMOID_DOMAIN).astype(F32))


def _max_rel(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))


def test_sigmoid_and_its_derivative_on_host_stay_within_the_derived_bounds():
    """Against float64 over |x| <= 80.  Bounds (tests/trainstats_ref.py): expf is documented to 1 ulp = 2 U relative (U = 2^-24);
    the sigmoid adds one rounding for the add and one for the divide: 4 U = 2.4e-7; the derivative t / (1 + t)^2 carries the
    add's rounding twice, a multiply and a divide: 6 U = 3.6e-7; the backward's term multiplies by the scale once more: 7 U."""
    lib = _shim()
    x = _sigmoid_inputs()
    out = np.empty_like(x)
    lib.hc_sigmoid(len(x), _p(x), _p(out))
    e_s = _max_rel(out, ref.sigmoid64(x))
    lib.hc_sigmoid_grad(len(x), _p(x), _p(out))
    e_g = _max_rel(out, ref.sigmoid_grad64(x))
    e_t = 0.0
    for scale in (F32(0.01) / F32(12345), F32(1.5)):
        lib.hc_alpha_regul_term(len(x), _p(x), scale, _p(out))
        want = ref.sigmoid_grad64(x) * np.float64(scale)
        normal = want >= np.finfo(F32).tiny   # a product below 2^-126 is a denormal: its rounding is absolute, not relative
        assert normal.sum() > 0.9 * len(x)
        e_t = max(e_t, _max_rel(out[normal], want[normal]))
        assert np.all(np.abs(out[~normal] - want[~normal]) <= np.finfo(F32).smallest_subnormal)
    print(f"\nmax relative error: sigmoid {e_s:.3e} (bound {ref.SIGMOID_REL:.3e}), derivative {e_g:.3e} "
          f"(bound {ref.SIGMOID_GRAD_REL:.3e}), backward term {e_t:.3e} (bound {ref.ALPHA_TERM_REL:.3e})")
    assert e_s <= ref.SIGMOID_REL
    assert e_g <= ref.SIGMOID_GRAD_REL
    assert e_t <= ref.ALPHA_TERM_REL


def test_derivative_form_is_the_product_s_one_minus_s():
    """t / (1 + t)^2 is s (1 - s): the restatement's two float64 forms agree where the product does not cancel."""
    x = np.linspace(-5, 5, 1001)
    s = ref.sigmoid64(x)
    assert np.allclose(ref.sigmoid_grad64(x), s * (1 - s), rtol=1e-13, atol=0)


def test_restatement_of_the_means():
    rng = np.random.default_rng(3)
    radii = rng.choice(np.array([0, 0, 0, 2, 9], np.int32), 50)
    op = rng.standard_normal((50, 1)).astype(F32)
    rest = rng.standard_normal((50, 15, 3)).astype(F32)
    r = ref.visible_means(radii, op, rest)
    t_mask = torch.from_numpy(radii) > 0
    assert r["n"] == int(t_mask.sum())
    assert abs(r["alpha_mean"] - float(torch.sigmoid(torch.from_numpy(op).double())[t_mask].abs().mean())) < 1e-14
    assert abs(r["sh_abs_mean"] - float(torch.from_numpy(rest).double()[t_mask].abs().mean())) < 1e-14
    none = ref.visible_means(np.zeros(5, np.int32), op[:5], rest[:5])
    assert none["n"] == 0 and np.isnan(none["alpha_mean"]) and np.isnan(none["sh_abs_mean"])
    assert np.isnan(ref.visible_means(radii, op, rest[:, :0])["sh_abs_mean"])   # M == 1: the mean of nothing


def test_module_signatures():
    assert list(inspect.signature(ts.visible_means).parameters) == ["radii", "opacity", "features_rest"]
    assert inspect.signature(ts.visible_means).parameters["opacity"].default is None
    assert inspect.signature(ts.visible_means).parameters["features_rest"].default is None
    assert list(inspect.signature(ts.add_densification_stats).parameters) == ["pc", "viewspace_point_tensor", "radii"]
    assert list(inspect.signature(ts.densification_stats).parameters) == ["viewspace_grad", "radii", "xyz_gradient_accum", "denom",
                                                                           "max_radii2D"]
    assert ts.VisibleMeans._fields == ("visibility_filter", "n_visible", "alpha_mean", "sh_abs_mean")


def test_module_never_reads_back_or_indexes_by_mask():
    src = open(ts.__file__).read()
    code = re.sub(r'""".*?"""', "", src, flags=re.S)
    code = re.sub(r"#.*", "", code)
    for banned in (".item(", ".cpu(", "nonzero", ".tolist(", ".numpy("):
        assert banned not in code, banned
    assert not re.search(r"[\w\)\]]\[[^\]]*(mask|vis|visibility_filter)[^\]]*\]", code)   # no boolean indexing


class _Model:
    def __init__(self, P, **kw):
        self.xyz_gradient_accum = kw.get("acc", torch.zeros(P, 1))
        self.denom = kw.get("den", torch.zeros(P, 1))
        self.max_radii2D = kw.get("mx", torch.zeros(P))


def test_host_tensors_are_refused():
    P = 8
    radii = torch.ones(P, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.visible_means(radii, opacity=torch.zeros(P, 1), features_rest=torch.zeros(P, 15, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.visible_means(radii)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.add_densification_stats(_Model(P), torch.zeros(P, 3), radii)
    from diff_gaussian_rasterization import _C
    for binding in ("ctypes", "torch"):
        was = _C.set_binding(binding)
        try:
            with pytest.raises(RuntimeError, match="no CPU path"):
                _C.visible_means(radii, torch.zeros(P, 1), None)
            with pytest.raises(RuntimeError, match="no CPU path"):
                _C.densification_stats(torch.zeros(P, 3), radii, torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P))
        finally:
            _C.set_binding(was)


@pytest.mark.parametrize("call,exc,match", [
    (lambda: ts.visible_means(torch.ones(8, dtype=torch.int64)), TypeError, "radii is torch.int64"),
    (lambda: ts.visible_means(torch.ones(8, 1, dtype=torch.int32)), ValueError, r"radii must be \[P\]"),
    (lambda: ts.visible_means(torch.ones(8, dtype=torch.int32), opacity=torch.zeros(8, 1, dtype=torch.float64)), TypeError,
     "opacity is torch.float64"),
    (lambda: ts.visible_means(torch.ones(8, dtype=torch.int32), opacity=torch.zeros(7, 1)), ValueError, "opacity must be"),
    (lambda: ts.visible_means(torch.ones(8, dtype=torch.int32), features_rest=torch.zeros(8, 45)), ValueError,
     "features_rest must be"),
    (lambda: ts.visible_means(torch.ones(8, dtype=torch.int32), features_rest=torch.zeros(8, 15, 3, dtype=torch.float16)),
     TypeError, "features_rest is torch.float16"),
    (lambda: ts.add_densification_stats(_Model(8, acc=torch.zeros(8, 1, dtype=torch.float64)), torch.zeros(8, 3),
                                        torch.ones(8, dtype=torch.int32)), TypeError, "xyz_gradient_accum is torch.float64"),
    (lambda: ts.add_densification_stats(_Model(8, den=torch.zeros(8)), torch.zeros(8, 3), torch.ones(8, dtype=torch.int32)),
     ValueError, r"denom must be \[8, 1\]"),
    (lambda: ts.add_densification_stats(_Model(8, mx=torch.zeros(8, dtype=torch.int32)), torch.zeros(8, 3),
                                        torch.ones(8, dtype=torch.int32)), TypeError, "max_radii2D is torch.int32"),
    (lambda: ts.add_densification_stats(_Model(8, mx=torch.zeros(16)[::2]), torch.zeros(8, 3), torch.ones(8, dtype=torch.int32)),
     ValueError, "max_radii2D is not contiguous"),
    (lambda: ts.add_densification_stats(_Model(8), torch.zeros(8, 2), torch.ones(8, dtype=torch.int32)), ValueError,
     "viewspace_grad must be"),
    (lambda: ts.add_densification_stats(_Model(8), torch.zeros(8, 3, requires_grad=True), torch.ones(8, dtype=torch.int32)),
     RuntimeError, "no .grad yet"),
])
def test_wrong_dtype_shape_or_layout_is_refused(call, exc, match):
    with pytest.raises(exc, match=match):
        call()


def test_header_declares_the_four_entry_points_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "r3dgs_trainstats.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(r3dgs_[a-z0-9_]+)\s*\(", code))
    assert names == {"r3dgs_train_stats_workspace_bytes", "r3dgs_visible_means", "r3dgs_alpha_regul_backward",
                     "r3dgs_densification_stats"}
    from diff_gaussian_rasterization import _C
    for n in names:
        assert hasattr(_C._lib, n), n
    assert _C._ext_loaded is not None
    for n in ("visible_means", "alpha_regul_backward", "densification_stats"):
        assert callable(getattr(_C._ext_loaded, n)) and callable(getattr(_C, n))


def test_workspace_query_and_argument_checks_need_no_gpu():
    """The size query is a function of P alone; NULL pointers and P <= 0 are answered before anything is launched."""
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    assert lib.r3dgs_train_stats_workspace_bytes(0) == 0 and lib.r3dgs_train_stats_workspace_bytes(-3) == 0
    for P in (1, 256, 257, 500_000):
        assert lib.r3dgs_train_stats_workspace_bytes(P) >= ((P + 255) // 256) * 20
    assert lib.r3dgs_visible_means(0, 16, None, None, None, None, None, None, None, None, None) == 0
    assert lib.r3dgs_alpha_regul_backward(-1, None, None, None, None, None, None) == 0
    assert lib.r3dgs_densification_stats(0, None, None, None, None, None, None) == 0
    assert lib.r3dgs_visible_means(5, 16, None, None, None, None, None, None, None, None, None) < 0
    assert b"NULL" in lib.r3dgs_last_error()
    assert lib.r3dgs_alpha_regul_backward(5, None, None, None, None, None, None) < 0
    assert b"NULL" in lib.r3dgs_last_error()
    assert lib.r3dgs_densification_stats(5, None, None, None, None, None, None) < 0
    assert b"NULL" in lib.r3dgs_last_error()
