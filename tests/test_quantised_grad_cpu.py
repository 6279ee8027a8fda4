"""CPU checks of the codebook-space fine-tune: the slot map of csrc/quant_math.h (quant_grad_slot, through
tests/hostcheck_quant_grad) against a numpy restatement of the decoder's layout, the C-ABI surface of
r3dgs_quantised_codebook_grad, QuantisedModel.to_ply -> from_ply on the golden files, and the host-side state of
requires_grad_ / parameters / commit.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import quant_grad_ref as gr
from tests import quant_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {True: "quantised_half_P200.ply", False: "quantised_P200.ply"}


@pytest.mark.parametrize("counts", qr.MIXES)
def test_slot_map_equals_the_numpy_restatement(counts):
    lib = gr.shim()
    m = qr.make_model(counts, seed=11 + sum(counts))
    got, want = gr.shim_slots(lib, m), gr.np_slots(m)
    assert got.shape == want.shape == (8 * sum(counts) + m["sh_ids"].size, 5)
    assert np.array_equal(got, want)   # the same triples, in (Gaussian, slot) order
    P, deg = sum(counts), np.repeat(np.arange(4), counts)
    # every owned element once, and no features_rest element above a Gaussian's degree
    owned = {"dc": np.ones((P, 1, 3), bool), "rest": np.arange(15)[None, :, None] < ((deg + 1) ** 2 - 1)[:, None, None],
             "opacity": np.ones((P, 1), bool), "scaling": np.ones((P, 3), bool), "rotation": np.ones((P, 4), bool)}
    for t, name in enumerate(gr.TENSORS):
        elems = got[got[:, 2] == t, 3]
        hits = np.bincount(elems, minlength=P * int(np.prod(gr.SHAPES[name])))
        mask = np.broadcast_to(owned[name], (P,) + gr.SHAPES[name]).reshape(-1)
        assert np.array_equal(hits, mask.astype(np.int64)), name
    # every id byte of the model is named once; the value read is the byte's
    at = got[:, 4]
    assert np.array_equal(np.sort(at[at >= 0]), np.arange(m["sh_ids"].size))
    assert np.array_equal(np.sort(-at[at < 0] - 1), np.arange(8 * P))
    assert np.array_equal(got[at >= 0, 1], m["sh_ids"][at[at >= 0]])
    assert np.array_equal(got[at < 0, 1], m["geom_ids"].reshape(-1)[-at[at < 0] - 1])
    # books: SH coefficient k -> book k; geometry -> 16, 17 x3, 18, 19 x3
    assert np.array_equal(np.bincount(got[at < 0, 0], minlength=20)[16:], np.array([1, 3, 1, 3]) * P)


def test_grid_is_a_function_of_P():
    from diff_gaussian_rasterization import _C
    lib = gr.shim()
    chunk, cap = lib.hqg_chunk(), lib.hqg_max_groups()
    assert (chunk, cap) == (_C.QUANTISED_GRAD_CHUNK, _C.QUANTISED_GRAD_MAX_GROUPS) and chunk % 64 == 0
    for P in (1, chunk - 1, chunk, chunk + 1, 3 * chunk - 17, cap * chunk, cap * chunk + 1, 6_000_000, 2 ** 31 - 1):
        chunks = -(-P // chunk)
        groups, per = lib.hqg_groups(P), lib.hqg_chunks_per_group(P)
        assert 1 <= groups <= cap and (groups - 1) * per < chunks <= groups * per, P
        assert per == 1 or chunks > cap
        assert _C._lib.r3dgs_quantised_codebook_grad_workspace_bytes(P) == groups * 20 * 256 * 8
    assert _C._lib.r3dgs_quantised_codebook_grad_workspace_bytes(0) == 0


def test_c_abi_surface():
    from diff_gaussian_rasterization import _C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r3dgs_quantised.h")).read(), flags=re.S)
    assert "hipStream_t" not in hdr and "torch" not in hdr and "at::" not in hdr and "#include <hip" not in hdr
    lib = C.CDLL(os.path.join(ROOT, "reduced-3dgs_amd", "libr3dgs_hip.so"))
    for n in ("r3dgs_quantised_codebook_grad_workspace_bytes", "r3dgs_quantised_codebook_grad"):
        assert hasattr(lib, n), f"{n} not exported"
    m = re.search(r"\bsize_t\s+r3dgs_quantised_codebook_grad_workspace_bytes\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "int P"
    m = re.search(r"\bint\s+r3dgs_quantised_codebook_grad\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "r3dgs_quantised_codebook_grad is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["int P", "const int* coeffsNum", "const int* perBandPrimitiveCount", "const int* cumSumPrimitiveCount",
                    "const unsigned char* geom_ids", "const unsigned char* sh_ids", "const float* dL_dfeatures_dc",
                    "const float* dL_dfeatures_rest", "const float* dL_dopacity", "const float* dL_dscaling",
                    "const float* dL_drotation", "float* dL_dcodebooks", "void* workspace", "void* stream"]
    assert len(_C._lib.r3dgs_quantised_codebook_grad.argtypes) == len(args)
    # both bindings expose it, and both refuse host tensors
    assert callable(_C.quantised_codebook_grad) and callable(_C._ext_loaded.quantised_codebook_grad)
    z = torch.zeros
    host = (z(4, 8, dtype=torch.uint8), z(12, dtype=torch.uint8), torch.tensor([4, 0, 0, 0], dtype=torch.int32),
            torch.tensor([4, 4, 4, 4], dtype=torch.int32), torch.tensor([1, 4, 9, 16], dtype=torch.int32), z(4, 1, 3), None, None,
            None, None)
    for name in ("torch", "ctypes"):
        was = _C.set_binding(name)
        try:
            with pytest.raises(RuntimeError, match="no CPU path"):
                _C.quantised_codebook_grad(*host)
        finally:
            _C.set_binding(was)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("half", [True, False])
def test_to_ply_from_ply_round_trip(tmp_path, half):
    from plyfile import PlyData
    from r3dgs_quantised import QuantisedModel
    src = os.path.join(GOLDEN, FILES[half])
    qm = QuantisedModel.from_ply(src, half_float=half, device="cpu")
    out = str(tmp_path / "sub" / "copy.ply")
    qm.to_ply(out, half)
    back = QuantisedModel.from_ply(out, half_float=half, device="cpu")
    assert back.per_band_count == qm.per_band_count
    for a, b in zip(qm.arrays(), back.arrays()):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    want, got = PlyData.read(src), PlyData.read(out)
    assert [e.name for e in got.elements] == [e.name for e in want.elements]
    for g, w in zip(got.elements, want.elements):
        assert g.count == w.count
        assert [(p.name, p.val_dtype) for p in g.properties] == [(p.name, p.val_dtype) for p in w.properties], g.name
        for p in w.properties:
            assert np.array_equal(np.asarray(g[p.name]), np.asarray(w[p.name])), (g.name, p.name)
    qm.to_ply(str(tmp_path / "default.ply"))   # the default format is the model's own
    assert open(str(tmp_path / "default.ply"), "rb").read() == open(out, "rb").read()


@pytest.mark.parametrize("half", [True, False])
def test_requires_grad_parameters_commit_host_state(half):
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(GOLDEN, FILES[half]), half_float=half, device="cpu")
    assert not qm.trainable and qm.parameters() == [] and qm.xyz_master is None
    stored = qm.xyz.clone()
    assert qm.requires_grad_(codebooks=True, xyz=True) is qm and qm.trainable
    assert qm.codebooks.is_leaf and qm.codebooks.requires_grad and qm.codebooks.dtype == torch.float32
    m = qm.xyz_master
    assert m.is_leaf and m.requires_grad and m.dtype == torch.float32 and tuple(m.shape) == (200, 3)
    assert np.array_equal(m.detach().numpy(), stored.numpy().astype(np.float32))   # the exact widening
    groups = qm.parameters()
    assert [g["name"] for g in groups] == ["codebooks", "xyz"]
    assert groups[0]["params"][0] is qm.codebooks and groups[1]["params"][0] is qm.xyz_master
    torch.optim.Adam(groups, lr=1e-3)   # the list is what an optimizer takes
    qm.requires_grad_(codebooks=True, xyz=False)
    assert qm.xyz_master is None and [g["name"] for g in qm.parameters()] == ["codebooks"]
    qm.requires_grad_(codebooks=False, xyz=True)
    assert [g["name"] for g in qm.parameters()] == ["xyz"] and not qm.codebooks.requires_grad
    qm.requires_grad_()
    with pytest.raises(RuntimeError, match="commit"):
        qm.to_ply("unused.ply")
    # training moves the leaves; the stored positions stay until commit
    rng = np.random.default_rng(5)
    with torch.no_grad():
        qm.xyz_master += torch.from_numpy(rng.normal(0, 1e-3, (200, 3)).astype(np.float32))
        qm.codebooks += torch.from_numpy(rng.normal(0, 1e-3, (20, 256)).astype(np.float32))
    assert torch.equal(_bits(qm.xyz), _bits(stored))
    master, books = qm.xyz_master.detach().clone(), qm.codebooks.detach().clone()
    qm.commit()
    assert qm.xyz_master is None and not qm.trainable and qm.parameters() == []
    assert not qm.codebooks.requires_grad and qm.codebooks.is_leaf and qm.xyz.dtype == stored.dtype
    if half:   # rounds as .half() does: numpy's conversion is round-to-nearest-even too
        assert np.array_equal(qm.xyz.numpy().view(np.uint16), master.numpy().astype(np.float16).view(np.uint16))
        assert np.array_equal(qm.codebooks.numpy(), books.numpy().astype(np.float16).astype(np.float32))
    else:
        assert torch.equal(qm.xyz, master) and torch.equal(qm.codebooks, books)
    qm.requires_grad_(codebooks=True, xyz=False)
    qm.commit(half_float=not half)   # the explicit choice overrides the default: kept as they are / rounded now
    assert np.array_equal(qm.codebooks.numpy(), books.numpy().astype(np.float16).astype(np.float32))
