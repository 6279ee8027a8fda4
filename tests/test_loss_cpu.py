"""CPU checks of the fused L1 + D-SSIM loss (reduced-3dgs_amd/r3dgs_loss.py, csrc/loss.hip, include/r3dgs_loss.h): the
float64 restatement the GPU tests compare against is pinned to the reference's recorded output, the window weights are the
reference's bit for bit, the per-pixel kernel arithmetic (csrc/loss_math.h) runs on the host through a test shim, and the
Python surface has the reference's signatures and refuses what it does not support.  No GPU needed."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import r3dgs_loss
from diff_gaussian_rasterization import _C
from tests import loss_ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_loss", "hostcheck_loss.hip")
SO = os.path.join(HERE, "hostcheck_loss", "libhostcheck_loss.so")


def _shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the loss host-check shim")
    lib.hc_ssim_c1.restype = C.c_float
    lib.hc_ssim_c2.restype = C.c_float
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_float64_restatement_reproduces_the_reference_fixture(golden_dir):
    """tests/golden/ref_loss_grad.npz holds the reference's l1_loss / ssim / loss / d loss / d image at 3x40x56
    (make_golden.py::ref_loss).  The float64 restatement every GPU comparison uses agrees with it to fp32 rounding."""
    d = np.load(os.path.join(golden_dir, "ref_loss_grad.npz"))
    r = loss_ref.evaluate(d["image"], d["gt"], torch.float64, lam=0.2)
    assert abs(r["ssim"] - float(d["ssim"])) <= 1.0e-8 * 1.5
    assert abs(r["l1"] - float(d["l1"])) <= 1e-7
    assert abs(r["loss"] - float(d["loss"])) <= 1e-7
    g = d["dloss_dimage"]
    assert np.abs(r["dloss"] - g).max() <= 7.5e-7 * 1.5 * np.abs(g).max()


def test_window_is_the_references_bit_for_bit():
    w = _C.ssim_window()
    assert w.dtype == np.float32 and w.shape == (11,)
    assert np.array_equal(w.view(np.uint32), loss_ref.window32().view(np.uint32))


def _ssim_pixel64(mx, my, exx, eyy, exy):
    mx, my, exx, eyy, exy = (np.asarray(v, np.float64) for v in (mx, my, exx, eyy, exy))
    c1, c2 = float(np.float32(loss_ref.C1)), float(np.float32(loss_ref.C2))
    a1, a2 = 2 * mx * my + c1, 2 * (exy - mx * my) + c2
    b1, b2 = mx * mx + my * my + c1, (exx - mx * mx) + (eyy - my * my) + c2
    s = a1 * a2 / (b1 * b2)
    t1, t2 = 2 * my * (a2 - a1) / (b1 * b2), 2 * mx * s * (b2 - b1) / (b1 * b2)
    d_mu = t1 - t2
    d_exx = -s / b2
    d_exy = 2 * a1 / (b1 * b2)
    return s, d_mu, d_exx, d_exy, np.abs(t1) + np.abs(t2)


def _moments(rng, n, near_zero_var):
    mx = rng.uniform(-0.5, 3.0, n)
    my = rng.uniform(-0.5, 3.0, n)
    if near_zero_var:
        vx, vy = rng.uniform(0, 1e-6, n), rng.uniform(0, 1e-6, n)
    else:
        vx, vy = rng.uniform(0, 1.0, n), rng.uniform(0, 1.0, n)
    cxy = rng.uniform(-1, 1, n) * np.sqrt(vx * vy)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f(mx), f(my), f(vx + mx * mx), f(vy + my * my), f(cxy + mx * my)


@pytest.mark.parametrize("near_zero_var", [False, True], ids=["textured", "near_zero_variance"])
def test_pixel_math_on_host_matches_float64(near_zero_var):
    """S and its three partials from csrc/loss_math.h, run on the CPU, against float64 on the same fp32 moments: <= 1e-5
    relative (for dS/dmu_x, a difference of two terms, relative to the larger of the result and the terms' magnitude)."""
    lib = _shim()
    assert lib.hc_ssim_c1() == np.float32(loss_ref.C1) and lib.hc_ssim_c2() == np.float32(loss_ref.C2)
    rng = np.random.default_rng(3 + near_zero_var)
    n = 20000
    mom = _moments(rng, n, near_zero_var)
    out = np.zeros((n, 4), np.float32)
    lib.hc_ssim_pixel(n, *(_p(m) for m in mom), _p(out))
    s, d_mu, d_exx, d_exy, mu_scale = _ssim_pixel64(*mom)
    rel = lambda got, ref, scale: np.abs(got - ref) / np.maximum(np.abs(ref), scale)  # noqa: E731
    assert rel(out[:, 0], s, 1e-30).max() <= 1e-5
    assert rel(out[:, 1], d_mu, mu_scale).max() <= 1e-5
    assert rel(out[:, 2], d_exx, 1e-30).max() <= 1e-5
    assert rel(out[:, 3], d_exy, 1e-30).max() <= 1e-5


def test_l1_sign_convention_on_host():
    lib = _shim()
    x = np.array([1.0, 0.0, -2.0, 0.5], np.float32)
    y = np.array([0.0, 0.0, -1.0, 0.5], np.float32)
    out = np.zeros(4, np.float32)
    lib.hc_l1_sign(4, _p(x), _p(y), _p(out))
    assert out.tolist() == [1.0, 0.0, -1.0, 0.0]   # torch: sign(0) = 0


def test_signatures_mirror_the_reference():
    assert list(inspect.signature(r3dgs_loss.l1_loss).parameters) == ["network_output", "gt"]
    sig = inspect.signature(r3dgs_loss.ssim)
    assert list(sig.parameters) == ["img1", "img2", "window_size", "size_average", "aggregate"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [11, True, True]
    sig = inspect.signature(r3dgs_loss.l1_dssim)
    assert list(sig.parameters) == ["image", "gt", "lambda_dssim"] and sig.parameters["lambda_dssim"].default == 0.2


def test_module_does_not_shadow_the_reference_utils():
    assert r3dgs_loss.__name__ == "r3dgs_loss" and "utils" not in r3dgs_loss.__file__.split(os.sep)


def test_refusals():
    a, b = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_loss.ssim(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_loss.l1_dssim(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_loss.l1_loss(a, b)
    with pytest.raises(TypeError, match="float32"):
        r3dgs_loss.ssim(a.half(), b.half())
    with pytest.raises(ValueError, match="window_size"):
        r3dgs_loss.ssim(a, b, window_size=13)
    with pytest.raises(RuntimeError, match="requires grad"):
        r3dgs_loss.ssim(a, b.requires_grad_())
    with pytest.raises(ValueError, match="size_average=False"):
        r3dgs_loss.ssim(torch.rand(3, 16, 16), torch.rand(3, 16, 16), size_average=False)
