"""CPU checks of the evaluation metrics (reduced-3dgs_amd/r3dgs_metrics.py, csrc/metrics.hip, include/r3dgs_metrics.h): the
float64 restatement the GPU tests compare against is pinned to the reference's recorded output, the per-sample arithmetic of
csrc/metrics_math.h runs on the host through a test shim and equals torch's CPU results bit for bit, the Python surface has
the reference's signatures and refuses what it does not support, and the library exports what the header declares.
No GPU needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import r3dgs_metrics
from tests import metrics_ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck_metrics", "hostcheck_metrics.hip")
SO = os.path.join(HERE, "hostcheck_metrics", "libhostcheck_metrics.so")
EPS32 = 2.0 ** -24   # unit roundoff of fp32


def _shim():
    return build_shim(SRC, SO, EXACT, "hipcc not available to build the metrics host-check shim")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ulp32(v):
    v = np.float32(abs(v))
    return float(np.nextafter(v, np.float32(np.inf)) - v)


def test_float64_restatement_reproduces_the_reference_fixture(golden_dir):
    """tests/golden/ref_metrics.npz holds the reference's psnr / mse / l1_loss / ssim at 3x40x56 as float32
    (make_metrics_golden.py).  The reference sums fp32 squares: each term carries three roundings (the difference, the
    square, its addition) and torch's blocked sum a few more, so its mse is within 8 x 2^-24 relative of the exact mean; a
    relative change r of the mse moves the PSNR by 10 log10(e) r dB, and sqrt, reciprocal, log10 and the product by 20
    each round the fp32 result once more: two ulps of the recorded value cover them."""
    d = np.load(os.path.join(golden_dir, "ref_metrics.npz"))
    image, gt = d["image"], d["gt"]
    assert image.dtype == np.float32 and image.shape == (3, 40, 56) and image.min() < 0 and image.max() > 1
    r = metrics_ref.row(image, gt, "f32", clamp=True, quantise=False)
    db = 10.0 * np.log10(np.e)
    rel = 8 * EPS32

    def psnr_bar(p):
        return db * rel + 2 * _ulp32(p)

    assert d["psnr_bchw"].dtype == np.float32 and d["psnr_bchw"].shape == (1, 1) and d["psnr_chw"].shape == (3, 1)
    assert abs(r["psnr_image"] - float(d["psnr_bchw"][0, 0])) <= psnr_bar(d["psnr_bchw"][0, 0])
    assert abs(r["mse"] - float(d["mse_bchw"][0, 0])) <= rel * r["mse"]
    for c in range(3):
        assert abs(r[f"mse_c{c}"] - float(d["mse_chw"][c, 0])) <= rel * r[f"mse_c{c}"]
    assert r["mse_c3"] == 0.0
    ref_mean = float(d["psnr_chw"].astype(np.float64).mean())
    assert abs(r["psnr_channels"] - ref_mean) <= max(psnr_bar(p) for p in d["psnr_chw"][:, 0])
    assert abs(r["l1"] - float(d["l1"])) <= rel * r["l1"]
    # an fp32 evaluation of the SSIM mean against float64: the bar DESIGN.md section 12 states
    assert abs(r["ssim"] - float(d["ssim"])) <= 1e-6
    # the drop-ins' restatement, on the clamped and on the raw images
    ci, cg = metrics_ref.clamp01(image), metrics_ref.clamp01(gt)
    for a, b, key in ((ci, cg, "chw"), (ci[None], cg[None], "bchw"), (image, gt, "raw_chw")):
        m, p = metrics_ref.row_mse(a, b), metrics_ref.row_psnr(a, b)
        assert m.shape == (a.shape[0],)
        for i in range(a.shape[0]):
            assert abs(m[i] - float(d["mse_" + key][i, 0])) <= rel * m[i]
            assert abs(p[i] - float(d["psnr_" + key][i, 0])) <= psnr_bar(d["psnr_" + key][i, 0])
    # the recorded bytes are the restatement's 8-bit rounding
    assert np.array_equal(metrics_ref.quantise8(image), d["bytes_chw"])


def _quantise_inputs():
    k = np.arange(256, dtype=np.float32)
    base = np.concatenate([k / np.float32(255.0), (k + np.float32(0.5)) / np.float32(255.0)])
    up = np.nextafter(base, np.float32(np.inf))
    down = np.nextafter(base, np.float32(-np.inf))
    tiny = np.float32(1e-45)   # the smallest subnormal
    extra = np.array([0.0, -0.0, -1e-8, -0.001, -0.5, -1.0, -3e38, 1.0000001, 1.002, 1.5, 2.0, 255.0, 256.0, 3e38, np.inf, -np.inf,
                      tiny, -tiny, 1e-40, -1e-40, 1.1754942e-38, 0.00196, 0.0019607844, 0.99803925, 0.998, 0.5], np.float32)
    return np.ascontiguousarray(np.concatenate([base, up, down, np.nextafter(up, np.float32(np.inf)),
                                                np.nextafter(down, np.float32(-np.inf)), extra]).astype(np.float32))


def test_quantise8_on_host_equals_torch_bit_for_bit():
    lib = _shim()
    x = _quantise_inputs()
    assert not np.isnan(x).any() and x.size > 2500
    got = np.zeros(x.size, np.uint8)
    lib.hc_quantise8(x.size, _p(x), _p(got))
    want = torch.from_numpy(x.copy()).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(got, want), x[got != want][:8]
    assert np.array_equal(metrics_ref.quantise8(x), want)   # and the restatement agrees with both
    assert len(set(got.tolist())) == 256
    # NaN: undefined in the reference (a float NaN converted to uint8), pinned to 0 here
    nan = np.array([np.nan, -np.nan], np.float32)
    out = np.full(2, 7, np.uint8)
    lib.hc_quantise8(2, _p(nan), _p(out))
    assert out.tolist() == [0, 0] and metrics_ref.quantise8(nan).tolist() == [0, 0]


def test_loads_on_host_equal_torch_bit_for_bit():
    lib = _shim()
    u = np.arange(256, dtype=np.uint8)
    got = np.zeros(256, np.float32)
    lib.hc_load_u8(256, _p(u), _p(got))
    want = torch.tensor(u, dtype=torch.uint8).float().div(255).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(metrics_ref.from_u8(u).view(np.uint32), want.view(np.uint32))
    x = np.concatenate([_quantise_inputs(), np.array([np.nan], np.float32)])
    out = np.zeros(x.size, np.float32)
    for flags, want in ((0, x), (1, torch.clamp(torch.from_numpy(x.copy()), 0.0, 1.0).numpy()),
                        (2, metrics_ref.from_u8(metrics_ref.quantise8(x))), (3, metrics_ref.from_u8(metrics_ref.quantise8(x)))):
        lib.hc_load_f32(x.size, _p(x), flags, _p(out))
        # -0.0 clamps to -0.0 in torch and to either zero here: equal as values; everything else bit for bit
        same = (out.view(np.uint32) == want.view(np.uint32)) | ((out == 0) & (want == 0))
        assert same.all(), (flags, x[~same][:8])
        assert np.array_equal(metrics_ref.load_image(x, bool(flags & 1), bool(flags & 2)), out, equal_nan=True)
    assert np.isnan(out[-1]) == False   # noqa: E712  (quantise mode: NaN -> 0)


def test_error_terms_on_host_are_exact_differences_in_double():
    lib = _shim()
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.2, 1.3, 4096).astype(np.float32)
    y = rng.uniform(0, 1, 4096).astype(np.float32)
    y[:16] = x[:16]
    a, s = np.zeros(4096), np.zeros(4096)
    lib.hc_err(4096, _p(x), _p(y), _p(a), _p(s))
    d = x.astype(np.float64) - y.astype(np.float64)
    assert np.array_equal(a, np.abs(d)) and np.array_equal(s, d * d) and (a[:16] == 0).all()


def test_signatures_mirror_the_reference():
    # utils/image_utils.py:14,17: mse(img1, img2), psnr(img1, img2)
    assert list(inspect.signature(r3dgs_metrics.mse).parameters) == ["img1", "img2"]
    assert list(inspect.signature(r3dgs_metrics.psnr).parameters) == ["img1", "img2"]
    sig = inspect.signature(r3dgs_metrics.image_metrics)
    assert list(sig.parameters) == ["image", "gt", "clamp", "quantise", "out"]
    assert [sig.parameters[k].default for k in ("clamp", "quantise", "out")] == [True, False, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("clamp", "quantise", "out"))
    sig = inspect.signature(r3dgs_metrics.evaluate)
    assert list(sig.parameters) == ["cameras", "model", "pipe", "background", "quantise", "render"]
    assert list(inspect.signature(r3dgs_metrics.to_uint8).parameters) == ["image"]
    assert r3dgs_metrics.FIELDS == metrics_ref.FIELDS and r3dgs_metrics.ROW == len(metrics_ref.FIELDS)
    assert "utils" not in r3dgs_metrics.__file__.split(os.sep)


def test_refusals():
    a, b = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    for fn in (r3dgs_metrics.mse, r3dgs_metrics.psnr, r3dgs_metrics.image_metrics):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_metrics.to_uint8(a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_metrics.image_metrics(a, (b * 255).to(torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_metrics.evaluate([object()], None, None, torch.zeros(3))
    with pytest.raises(TypeError, match="float32"):
        r3dgs_metrics.psnr(a.half(), b.half())
    with pytest.raises(TypeError, match="float32"):
        r3dgs_metrics.image_metrics(a.double(), b)
    with pytest.raises(TypeError, match="float32 or uint8"):
        r3dgs_metrics.image_metrics(a, b.half())
    with pytest.raises(ValueError, match="shapes differ"):
        r3dgs_metrics.mse(a, torch.rand(3, 16, 15))
    with pytest.raises(ValueError, match="shapes differ"):
        r3dgs_metrics.image_metrics(a, torch.rand(3, 16, 15))
    with pytest.raises(ValueError, match="shapes differ"):
        r3dgs_metrics.image_metrics(a, torch.zeros(16, 3, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="ambiguous"):
        r3dgs_metrics.image_metrics(torch.rand(3, 3, 3), torch.zeros(3, 3, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1 <= C <= 4"):
        r3dgs_metrics.image_metrics(torch.rand(5, 8, 8), torch.rand(5, 8, 8))
    with pytest.raises(ValueError, match="1 <= C <= 4"):
        r3dgs_metrics.to_uint8(torch.rand(1, 3, 8, 8))
    with pytest.raises(ValueError, match="no cameras"):
        r3dgs_metrics.evaluate([], None, None, torch.zeros(3))


def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    """Shapes, C > 4, unknown layouts, unknown flag bits and NULL pointers come back as < 0 with a message; none of these
    calls reaches a launch, so they run without a GPU."""
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    one = C.c_void_p(8)   # never dereferenced: every call below is refused first
    assert lib.r3dgs_image_metrics_workspace_bytes(3, 17, 70) == 3 * 2 * 2 * 3 * 8
    assert lib.r3dgs_image_metrics_workspace_bytes(5, 8, 8) == 0 and lib.r3dgs_image_metrics_workspace_bytes(3, 0, 8) == 0
    assert lib.r3dgs_row_mse_workspace_bytes(5, 7) == 5 * 8 and lib.r3dgs_row_mse_workspace_bytes(2, 4097) == 2 * 2 * 8
    assert lib.r3dgs_row_mse_workspace_bytes(0, 7) == 0 and lib.r3dgs_row_mse_workspace_bytes(1 << 31, 1) == 0
    for args, msg in (((5, 8, 8, one, one, 0, 0, one, one, None), "1 <= C <= 4"), ((3, 8, 0, one, one, 0, 0, one, one, None), "H, W >= 1"),
                      ((3, 8, 8, one, one, 3, 0, one, one, None), "layout"), ((3, 8, 8, one, one, 0, 4, one, one, None), "flag"),
                      ((3, 8, 8, None, one, 0, 0, one, one, None), "NULL"), ((3, 8, 8, one, None, 0, 0, one, one, None), "NULL"),
                      ((3, 8, 8, one, one, 0, 0, None, one, None), "NULL"), ((3, 8, 8, one, one, 0, 0, one, None, None), "NULL")):
        assert lib.r3dgs_image_metrics(*args) < 0
        assert msg in lib.r3dgs_last_error().decode()
    for args, msg in (((0, 4, one, one, one, one, None), "R, n >= 1"), ((4, 0, one, one, one, one, None), "R, n >= 1"),
                      ((4, 4, None, one, one, one, None), "NULL"), ((4, 4, one, one, None, one, None), "NULL")):
        assert lib.r3dgs_row_mse(*args) < 0
        assert msg in lib.r3dgs_last_error().decode()
    for args, msg in (((5, 8, 8, one, one, None), "1 <= C <= 4"), ((3, -1, 8, one, one, None), "H, W >= 1"),
                      ((3, 8, 8, None, one, None), "NULL"), ((3, 8, 8, one, None, None), "NULL")):
        assert lib.r3dgs_image_to_uint8(*args) < 0
        assert msg in lib.r3dgs_last_error().decode()


def test_header_symbols_are_exported():
    """The method of tests/test_capi_exports.py for include/r3dgs_metrics.h."""
    from diff_gaussian_rasterization import _C
    hdr = open(os.path.join(ROOT, "include", "r3dgs_metrics.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(r3dgs_[a-z0-9_]+)\s*\(", code))
    assert names == {"r3dgs_image_metrics_workspace_bytes", "r3dgs_image_metrics", "r3dgs_row_mse_workspace_bytes",
                     "r3dgs_row_mse", "r3dgs_image_to_uint8"}
    lib = C.CDLL(_C.LIBRARY_PATH)
    for n in sorted(names):
        assert hasattr(lib, n), f"{n} declared in the header but not exported"
    assert "hipStream_t" not in code and "#include <hip" not in code
    consts = dict(re.findall(r"#define\s+(R3DGS_[A-Z0-9_]+)\s+(\d+)", code))
    assert int(consts["R3DGS_METRICS_ROW"]) == _C.METRICS_ROW == len(r3dgs_metrics.FIELDS)
    assert (int(consts["R3DGS_GT_F32_CHW"]), int(consts["R3DGS_GT_U8_CHW"]), int(consts["R3DGS_GT_U8_HWC"])) == \
        (_C.GT_F32_CHW, _C.GT_U8_CHW, _C.GT_U8_HWC)
    assert (int(consts["R3DGS_METRICS_CLAMP"]), int(consts["R3DGS_METRICS_QUANTISE8"])) == (_C.METRICS_CLAMP, _C.METRICS_QUANTISE8)
    for name, idx in (("l1", "L1"), ("mse", "MSE"), ("mse_c0", "MSE_C"), ("psnr_image", "PSNR_IMAGE"),
                      ("psnr_channels", "PSNR_CHANNELS"), ("ssim", "SSIM")):
        assert r3dgs_metrics.FIELDS.index(name) == int(consts["R3DGS_METRICS_" + idx])
