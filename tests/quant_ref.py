"""Shared by tests/test_quantised_cpu.py and tests/test_quantised_gpu.py: seeded quantised models as numpy arrays, a numpy
restatement of the decode written from the format's description (not from quant_math.h), and the host-check shim."""
import ctypes as C
import os

import numpy as np
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck_quant", "hostcheck_quant.hip")
SO = os.path.join(HERE, "hostcheck_quant", "libhostcheck_quant.so")

# per-degree counts the issue names
MIXES = [(37, 0, 150, 70), (0, 0, 0, 300), (300, 0, 0, 0), (1, 1, 1, 1), (63, 65, 1, 130), (64, 64, 64, 64)]
KEYS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_degrees")
# halves every conversion has to get right: +-0, smallest / largest subnormal, smallest normal, largest finite, one
SPECIAL_HALVES = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x3C00], np.uint16)


def shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the quantised host-check shim")
    lib.hq_sh_bytes.restype = C.c_longlong
    lib.hq_model_bytes.restype = C.c_longlong
    lib.hq_model_bytes.argtypes = [C.c_longlong, C.c_void_p, C.c_int]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def tables(counts):
    per = np.array(counts, np.int32)
    return np.array([1, 4, 9, 16], np.int32), per, np.cumsum(per).astype(np.int32)


def make_model(counts, seed=0, half_xyz=True, half_centres=False, spread=0.6, centre=(0.0, 0.0, 0.0)):
    """A random quantised model with `counts` Gaussians of degree 0..3 -> dict(xyz, geom_ids, sh_ids, codebooks, counts).
    The cloud sits around `centre` (world units of the golden cameras); opacities, scales and colours are in the ranges a
    trained model has, so that a render of it has something to show.  half_centres: the codebooks hold half values (as a
    half_float file's), with the special halves among them."""
    rng = np.random.default_rng(seed)
    P = int(sum(counts))
    xyz = (rng.normal(0, spread, (P, 3)) + np.array(centre)).astype(np.float32)
    xyz = xyz.astype(np.float16) if half_xyz else xyz
    geom = rng.integers(0, 256, (P, 8), dtype=np.uint8)
    nsh = sum(3 * (d + 1) ** 2 * c for d, c in enumerate(counts))
    sh = rng.integers(0, 256, nsh, dtype=np.uint8)
    books = np.empty((20, 256), np.float32)
    books[0] = rng.normal(0.5, 1.0, 256)
    books[1:16] = rng.normal(0, 0.3, (15, 256))
    books[16] = rng.normal(0, 2.0, 256)            # opacity logits
    books[17] = rng.normal(-2.6, 0.5, 256)         # log-scales
    books[18] = rng.normal(0, 1, 256)
    books[19] = rng.normal(0, 1, 256)
    if half_centres:
        books = books.astype(np.float16)
        books[:16, :len(SPECIAL_HALVES)] = SPECIAL_HALVES.view(np.float16)   # SH books only: the geometry stays renderable
        books = books.astype(np.float32)
    return dict(xyz=xyz, geom_ids=geom, sh_ids=sh, codebooks=books, counts=tuple(int(c) for c in counts))


def np_decode(m):
    """What the reference's load_ply returns for the model, from the description of the format: rows sorted by degree,
    3 (d+1)^2 id bytes per Gaussian as [coefficient][channel]; coefficient k reads book k; coefficients the Gaussian does not
    store read centre 0 of their book; geometry ids are opacity, scale xyz, rotation re, rotation im xyz."""
    counts, books, geom = m["counts"], m["codebooks"], m["geom_ids"].astype(np.int64)
    P = sum(counts)
    feats = np.empty((P, 16, 3), np.float32)
    first = byte = 0
    for d, c in enumerate(counts):
        K = (d + 1) ** 2
        ids = m["sh_ids"][byte:byte + 3 * K * c].reshape(c, K, 3).astype(np.int64)
        for k in range(16):
            feats[first:first + c, k, :] = books[k][ids[:, k, :]] if k < K else books[k][0]
        first, byte = first + c, byte + 3 * K * c
    assert byte == m["sh_ids"].size
    return {"_xyz": m["xyz"].astype(np.float32), "_features_dc": feats[:, :1].copy(), "_features_rest": feats[:, 1:].copy(),
            "_opacity": books[16][geom[:, 0:1]], "_scaling": books[17][geom[:, 1:4]],
            "_rotation": np.concatenate([books[18][geom[:, 4:5]], books[19][geom[:, 5:8]]], axis=1),
            "_degrees": np.repeat(np.arange(4, dtype=np.int32), counts).reshape(P, 1)}


def shim_decode(lib, m):
    """quant_math.h's quant_decode_one over the model, on the host."""
    coeffs, per, cum = tables(m["counts"])
    P = sum(m["counts"])
    xyz = np.ascontiguousarray(m["xyz"])
    out = {"_xyz": np.full((P, 3), np.nan, np.float32), "_features_dc": np.full((P, 1, 3), np.nan, np.float32),
           "_features_rest": np.full((P, 15, 3), np.nan, np.float32), "_opacity": np.full((P, 1), np.nan, np.float32),
           "_scaling": np.full((P, 3), np.nan, np.float32), "_rotation": np.full((P, 4), np.nan, np.float32),
           "_degrees": np.full((P, 1), -1, np.int32)}
    lib.hq_decode(P, _p(coeffs), _p(per), _p(cum), _p(xyz), int(xyz.dtype == np.float16), _p(np.ascontiguousarray(m["geom_ids"])),
                  _p(np.ascontiguousarray(m["sh_ids"])), _p(np.ascontiguousarray(m["codebooks"])), *(_p(out[k]) for k in KEYS))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def model_arrays(qm):
    """QuantisedModel (host or device) -> the dict of numpy arrays make_model returns."""
    return dict(xyz=qm.xyz.cpu().numpy(), geom_ids=qm.geom_ids.cpu().numpy(), sh_ids=qm.sh_ids.cpu().numpy(),
                codebooks=qm.codebooks.cpu().numpy(), counts=tuple(qm.per_band_count))
