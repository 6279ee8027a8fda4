"""CPU checks of the quantised (codebook-indexed) model: csrc/quant_math.h through tests/hostcheck_quant against a numpy
restatement of the format, r3dgs_quantised.QuantisedModel.from_ply on files the reference's own save_ply wrote
(tests/golden/quantised*_P200.ply, expected tensors: its load_ply's, quantised_P200_loaded.npz), the resident size, the C-ABI
surface of include/r3dgs_quantised.h and the refusals.  Everything here is exact: a lookup copies a float and every half is
a float.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import quant_ref as qr
from tests.quant_ref import _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"   # as tests/test_plyfile_shim.py: only present where the suite is authored
NEW = ("r3dgs_quantised_forward", "r3dgs_quantised_forward_reserved", "r3dgs_quantised_decode", "r3dgs_quantised_bytes")
FILES = {True: "quantised_half_P200.ply", False: "quantised_P200.ply"}


def assert_same(got, want, what=""):
    for k in qr.KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(qr.bits(g), qr.bits(w)), (what, k)


def test_half_to_float_every_pattern():
    lib = qr.shim()
    h = np.arange(65536, dtype=np.uint16)
    out = np.empty(65536, np.float32)
    lib.hq_half_to_float(65536, _p(h), _p(out))
    want = h.view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(out), nan) and int(nan.sum()) == 2046
    assert np.array_equal(out.view(np.uint32)[~nan], want.view(np.uint32)[~nan])   # +-0, subnormals, 65504, +-inf included
    for s in qr.SPECIAL_HALVES:
        assert out.view(np.uint32)[s] == want.view(np.uint32)[s]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("counts", qr.MIXES)
def test_shim_decode_equals_the_numpy_restatement(counts, half):
    lib = qr.shim()
    m = qr.make_model(counts, seed=sum(counts) + int(half), half_xyz=half, half_centres=half)
    if half:   # the special halves among the positions too
        m["xyz"].reshape(-1)[:len(qr.SPECIAL_HALVES)] = qr.SPECIAL_HALVES.view(np.float16)[:m["xyz"].size]
    assert_same(qr.shim_decode(lib, m), qr.np_decode(m), counts)
    # addressing on its own: where each row starts, and which degree it has
    coeffs, per, cum = qr.tables(counts)
    P = sum(counts)
    off, deg = np.empty(P, np.int32), np.empty(P, np.int32)
    lib.hq_ragged_offsets(P, _p(coeffs), _p(per), _p(cum), _p(off), _p(deg))
    want_deg = np.repeat(np.arange(4), counts)
    assert np.array_equal(deg, want_deg)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum((want_deg + 1) ** 2)[:-1]]))
    assert lib.hq_sh_bytes(_p(coeffs), _p(per)) == m["sh_ids"].size
    # the row the colour kernel's accessor hands to sh_to_rgb: dense-row order, DC rgb first
    dec = qr.np_decode(m)
    for i in (0, P // 2, P - 1):
        row = np.full(48, np.nan, np.float32)
        d = lib.hq_sh_row(i, _p(coeffs), _p(per), _p(cum), _p(m["sh_ids"]), _p(m["codebooks"]), _p(row))
        n = 3 * (d + 1) ** 2
        full = np.concatenate([dec["_features_dc"][i], dec["_features_rest"][i]]).reshape(-1)
        assert d == want_deg[i] and np.array_equal(qr.bits(row[:n]), qr.bits(full[:n])) and np.isnan(row[n:]).all()


@pytest.mark.parametrize("half", [True, False])
def test_from_ply_on_the_reference_written_fixture(half):
    from r3dgs_quantised import QuantisedModel
    lib = qr.shim()
    qm = QuantisedModel.from_ply(os.path.join(GOLDEN, FILES[half]), half_float=half, device="cpu")
    assert qm.per_band_count == [37, 13, 80, 70] and qm.P == 200 and qm.xyz_is_half == half
    assert qm.max_sh_degree == 3 and qm.active_sh_degree == 3
    assert qm.xyz.dtype == (torch.float16 if half else torch.float32) and qm.geom_ids.dtype == torch.uint8
    assert qm.sh_ids.numel() == 3 * (37 + 4 * 13 + 9 * 80 + 16 * 70) and tuple(qm.codebooks.shape) == (20, 256)
    want = np.load(os.path.join(GOLDEN, "quantised_P200_loaded.npz"))
    pre = "half" if half else "float"
    assert_same(qr.shim_decode(lib, qr.model_arrays(qm)), {k: want[pre + k] for k in qr.KEYS}, FILES[half])
    with pytest.raises(RuntimeError, match="no CPU path"):   # a host-resident model holds the arrays; nothing computes on it
        qm.decode()


# ---------------------------------------------------------------------------------- the reference's code on the shim
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "scene")),
                               reason="reference tree only exists in the authoring container")


@pytest.fixture()
def ref_gm(monkeypatch):
    monkeypatch.syspath_prepend(REF)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    if not hasattr(np, "cast"):   # np.cast[np.float16](..) (gaussian_model.py:269) left NumPy in 2.0
        class _Cast:
            def __getitem__(self, dtype):
                return lambda a: np.asarray(a, dtype=dtype)
        monkeypatch.setattr(np, "cast", _Cast(), raising=False)
    mods = lambda: [k for k in sys.modules if k.split(".")[0] in ("scene", "utils")]   # noqa: E731
    for m in mods():
        monkeypatch.delitem(sys.modules, m)
    import scene.gaussian_model as gm
    yield gm
    for m in mods():
        sys.modules.pop(m, None)


def _ref_model(gm, P=700, seed=3):
    """As tests/test_plyfile_shim.py::_model, with random codebooks."""
    g = torch.Generator().manual_seed(seed)
    m = gm.GaussianModel(3)
    m._degrees = torch.randint(0, 4, (P, 1), generator=g, dtype=torch.int32)
    m._xyz = torch.randn(P, 3, generator=g)

    def book(cols):
        return gm.Codebook(torch.randint(0, 256, (P, cols), generator=g, dtype=torch.uint8), torch.randn(256, 1, generator=g))
    cb = OrderedDict()
    cb["features_dc"] = book(3)
    for i in range(15):
        cb[f"features_rest_{i}"] = book(3)
    cb["opacity"], cb["scaling"], cb["rotation_re"], cb["rotation_im"] = book(1), book(3), book(1), book(3)
    m._codebook_dict = cb
    return m


@needs_ref
@pytest.mark.parametrize("half", [False, True])
def test_reference_save_ply_from_ply_decode_equals_reference_load_ply(ref_gm, tmp_path, half):
    from r3dgs_quantised import QuantisedModel
    lib = qr.shim()
    m = _ref_model(ref_gm)
    path = str(tmp_path / "point_cloud_quantised.ply")
    m.save_ply(path, quantised=True, half_float=half)
    back = ref_gm.GaussianModel(3)
    back.load_ply(path, half_float=half, quantised=True)
    want = {k: getattr(back, k).detach().numpy() for k in qr.KEYS}
    qm = QuantisedModel.from_ply(path, half_float=half, device="cpu")
    assert_same(qr.shim_decode(lib, qr.model_arrays(qm)), want, "from_ply")
    # and built from the model in memory: the same arrays as from its file
    qg = QuantisedModel.from_gaussian_model(m, half_float=half)
    for a, b in zip(qm.arrays(), qg.arrays()):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a,
                                                  b.view(torch.int16) if b.dtype == torch.float16 else b)


# ---------------------------------------------------------------------------------- size, surface, refusals
@pytest.mark.parametrize("half", [True, False])
@pytest.mark.parametrize("counts", qr.MIXES + [(0, 0, 0, 1000000)])
def test_resident_size(counts, half):
    from diff_gaussian_rasterization import _C
    lib = qr.shim()
    P = sum(counts)
    want = P * (8 + (6 if half else 12)) + sum(3 * (d + 1) ** 2 * c for d, c in enumerate(counts)) + 20 * 256 * 4 + 3 * 4 * 4
    assert _C.quantised_bytes(P, counts, half) == want   # no padding anywhere
    assert lib.hq_model_bytes(P, _p(np.array(counts, np.int32)), int(half)) == want
    if counts[3] == P and P >= 1000000:   # all degree 3: 62 B (half) against 236 B dense, plus the tables
        dense = P * 59 * 4
        assert want <= (0.27 if half else 0.29) * dense   # 62 / 236 = 0.263; float positions: 68 / 236 = 0.288
    with pytest.raises(RuntimeError, match="add up"):
        _C.quantised_bytes(P + 1, counts, half)


def test_nbytes_of_a_model_is_the_sum_of_its_arrays():
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(GOLDEN, FILES[True]), half_float=True, device="cpu")
    arrays = sum(t.numel() * t.element_size() for t in qm.arrays())
    assert qm.nbytes == arrays == 200 * 14 + qm.sh_ids.numel() + 20480 + 48


def _decl(hdr, name):
    m = re.search(r"\b(?:int|long long|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, f"{name} is not declared in include/r3dgs_quantised.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_c_abi_surface():
    from diff_gaussian_rasterization import _C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3dgs_quantised.h")).read(), flags=re.S)
    ras = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3dgs_rasterizer.h")).read(), flags=re.S)
    assert "hipStream_t" not in hdr and "torch" not in hdr
    lib = C.CDLL(os.path.join(ROOT, "reduced-3dgs_amd", "libr3dgs_hip.so"))
    for n in NEW:
        assert hasattr(lib, n), f"{n} not exported"
    model = ["const void* xyz", "int xyz_is_half", "const unsigned char* geom_ids", "const unsigned char* sh_ids",
             "const float* codebooks"]
    # the two forwards mirror the inference forwards argument for argument: the five model pointers become the quantised
    # arrays, colors_precomp / cov3D_precomp are gone
    for q, r in (("r3dgs_quantised_forward", "r3dgs_inference_forward"),
                 ("r3dgs_quantised_forward_reserved", "r3dgs_inference_forward_reserved")):
        m = re.search(r"\b(?:int|long long)\s+" + r + r"\s*\(([^;]*?)\)\s*;", ras, flags=re.S)
        ref_args = [" ".join(a.split()) for a in m.group(1).split(",")]
        want, placed = [], False
        for a in ref_args:
            name = a.split()[-1].lstrip("*")
            if name in ("means3D", "shs", "opacities", "scales", "rotations"):
                if not placed:
                    want += model
                    placed = True
            elif name not in ("colors_precomp", "cov3D_precomp"):
                want.append(a)
        assert _decl(hdr, q) == want, q
        assert len(getattr(_C._lib, q).argtypes) == len(want)
    dec = _decl(hdr, "r3dgs_quantised_decode")
    assert dec[:4] == ["int P", "const int* coeffsNum", "const int* perBandPrimitiveCount", "const int* cumSumPrimitiveCount"]
    assert dec[4:9] == model and dec[-1] == "void* stream"
    assert [a.split()[-1].lstrip("*") for a in dec[9:-1]] == ["xyz_out", "features_dc", "features_rest", "opacity", "scaling",
                                                              "rotation", "degrees"]
    assert len(_C._lib.r3dgs_quantised_decode.argtypes) == len(dec)
    assert _decl(hdr, "r3dgs_quantised_bytes") == ["int P", "const int* perBandPrimitiveCount_host", "int xyz_is_half"]
    for name in ("rasterize_gaussians_quantised", "quantised_decode", "quantised_bytes"):
        assert callable(getattr(_C, name))
    params = [p for p in inspect.signature(_C.rasterize_gaussians_quantised).parameters.values() if p.default is p.empty]
    assert [p.name for p in params] == ["background", "xyz", "geom_ids", "sh_ids", "codebooks", "scale_modifier", "viewmatrix",
                                        "projmatrix", "tan_fovx", "tan_fovy", "image_height", "image_width",
                                        "perBandPrimitiveCount", "cumSumPrimitiveCount", "coeffsNum", "campos", "prefiltered",
                                        "debug"]


def _write_ply(path, counts, centres=256, with_books=True, bands=4):
    """A file shaped like save_ply(quantised=True, half_float=False)'s, through this repository's plyfile."""
    from plyfile import PlyData, PlyElement
    from r3dgs_quantised import BOOK_NAMES
    els = []
    for d in range(bands):
        cn = (d + 1) ** 2 - 1
        dt = ([(k, "f4") for k in "xyz"] + [(f"f_dc_{i}", "u1") for i in range(3)] + [(f"f_rest_{i}", "u1") for i in range(3 * cn)] +
              [("opacity", "u1")] + [(f"scale_{i}", "u1") for i in range(3)] + [(f"rot_{i}", "u1") for i in range(4)])
        els.append(PlyElement.describe(np.zeros(counts[d], dtype=dt), f"vertex_{d}"))
    if with_books:
        els.append(PlyElement.describe(np.zeros(centres, dtype=[(n, "f4") for n in BOOK_NAMES]), "codebook_centers"))
    PlyData(els).write(str(path))


def test_refusals(tmp_path):
    from diff_gaussian_rasterization import _C
    from r3dgs_quantised import QuantisedModel
    ok = tmp_path / "ok.ply"
    _write_ply(ok, (2, 1, 0, 3))
    qm = QuantisedModel.from_ply(str(ok), half_float=False, device="cpu")
    assert qm.per_band_count == [2, 1, 0, 3] and qm.sh_ids.numel() == 3 * (2 + 4 + 48)
    _write_ply(tmp_path / "plain.ply", (2, 1, 0, 3), with_books=False)
    with pytest.raises(ValueError, match="no codebook_centers element"):
        QuantisedModel.from_ply(str(tmp_path / "plain.ply"), half_float=False, device="cpu")
    _write_ply(tmp_path / "c128.ply", (2, 1, 0, 3), centres=128)
    with pytest.raises(ValueError, match="only 256 are supported"):
        QuantisedModel.from_ply(str(tmp_path / "c128.ply"), half_float=False, device="cpu")
    _write_ply(tmp_path / "b3.ply", (2, 1, 0), bands=3)
    with pytest.raises(ValueError, match="4 bands"):
        QuantisedModel.from_ply(str(tmp_path / "b3.ply"), half_float=False, device="cpu")
    with pytest.raises(ValueError, match="4 bands"):
        QuantisedModel.from_ply(str(ok), half_float=False, max_sh_degree=2, device="cpu")
    # host tensors: refused loudly, no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.rasterize_gaussians_quantised(torch.zeros(3), *qm.arrays()[:4], 1.0, torch.eye(4), torch.eye(4), 1.0, 1.0, 16, 16,
                                         qm.per_band, qm.cumsum, qm.coeffs, torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.quantised_decode(*qm.arrays())
    # render() refuses what a quantised model cannot honour, before anything touches a device
    import r3dgs_render
    from types import SimpleNamespace as NS
    cam = NS(image_height=16, image_width=16, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4),
             full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))
    pipe = dict(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    with pytest.raises(ValueError, match="override_color is not supported"):
        r3dgs_render.render(cam, qm, NS(**pipe), torch.zeros(3), override_color=torch.zeros(6, 3))
    with pytest.raises(ValueError, match="compute_cov3D_python is not supported"):
        r3dgs_render.render(cam, qm, NS(**dict(pipe, compute_cov3D_python=True)), torch.zeros(3))
    with pytest.raises(ValueError, match="convert_SHs_python is not supported"):
        r3dgs_render.render(cam, qm, NS(**dict(pipe, convert_SHs_python=True)), torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r3dgs_render.render(cam, qm, NS(**pipe), torch.zeros(3))
