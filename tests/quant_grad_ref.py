"""Shared by tests/test_quantised_grad_cpu.py and tests/test_quantised_grad_gpu.py: the slot enumeration of the codebook
gradient derived in numpy from tests/quant_ref.np_decode's layout (not from quant_math.h), the float64 per-centre sums over
it, the error bar of "double accumulation, one rounding", and the host-check shim of quant_math.h's quant_grad_slot."""
import ctypes as C
import os

import numpy as np

from tests import quant_ref as qr
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_quant_grad", "hostcheck_quant_grad.hip")
SO = os.path.join(HERE, "hostcheck_quant_grad", "libhostcheck_quant_grad.so")
TENSORS = ("dc", "rest", "opacity", "scaling", "rotation")   # QuantGradTensor of quant_math.h
SHAPES = {"dc": (1, 3), "rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the codebook-gradient host-check shim")
    lib.hqg_enumerate.restype = C.c_longlong
    return lib


def shim_slots(lib, m):
    """quant_math.h's enumeration -> rows (book, id, tensor, elem, id_at), in (Gaussian, slot) order."""
    coeffs, per, cum = qr.tables(m["counts"])
    P = sum(m["counts"])
    cap = P * lib.hqg_slots()
    book, idv, tensor = (np.full(cap, -1, np.int32) for _ in range(3))
    elem, id_at = (np.full(cap, -1, np.int64) for _ in range(2))
    geom, sh = np.ascontiguousarray(m["geom_ids"]), np.ascontiguousarray(m["sh_ids"])
    sh_arg = sh if sh.size else np.zeros(1, np.uint8)
    n = lib.hqg_enumerate(P, qr._p(coeffs), qr._p(per), qr._p(cum), qr._p(geom), qr._p(sh_arg), qr._p(book), qr._p(idv),
                          qr._p(tensor), qr._p(elem), qr._p(id_at))
    return np.stack([book[:n], idv[:n], tensor[:n], elem[:n], id_at[:n]], axis=1).astype(np.int64)


def np_slots(m):
    """The same rows from the format's description, as np_decode lays the model out: Gaussians sorted by degree; 3 (d+1)^2
    id bytes each, [coefficient][channel]; coefficient k reads book k and lands in features_dc (k = 0) or row k - 1 of
    features_rest; geometry ids are opacity (book 16), scale xyz (17), rotation re (18), rotation im xyz (19)."""
    rows, first, byte = [], 0, 0
    geom = m["geom_ids"].astype(np.int64)
    for d, c in enumerate(m["counts"]):
        K = (d + 1) ** 2
        ids = m["sh_ids"][byte:byte + 3 * K * c].reshape(c, K, 3).astype(np.int64)
        for j in range(c):
            i = first + j
            rows.append((16, geom[i, 0], 2, i, -(8 * i + 0) - 1))
            rows += [(17, geom[i, 1 + k], 3, 3 * i + k, -(8 * i + 1 + k) - 1) for k in range(3)]
            rows.append((18, geom[i, 4], 4, 4 * i, -(8 * i + 4) - 1))
            rows += [(19, geom[i, 5 + k], 4, 4 * i + 1 + k, -(8 * i + 5 + k) - 1) for k in range(3)]
            for k in range(K):
                for ch in range(3):
                    at = byte + (j * K + k) * 3 + ch
                    rows.append((k, ids[j, k, ch], 0, 3 * i + ch, at) if k == 0 else
                                (k, ids[j, k, ch], 1, 45 * i + 3 * (k - 1) + ch, at))
        first, byte = first + c, byte + 3 * K * c
    return np.array(rows, np.int64).reshape(-1, 5)


def make_grads(P, seed, kind="wide"):
    """The five gradient tensors, float32, shaped as the decoder's outputs.  wide: mixed signs, magnitudes spread over
    2^-20 .. 2^20 (cancellation shows float accumulation), with +-0 and denormals sprinkled in."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in TENSORS:
        shape = (P,) + SHAPES[name]
        v = rng.standard_normal(shape) * np.exp2(rng.uniform(-20, 20, shape))
        v = v.astype(np.float32)
        if kind == "wide":
            pick = rng.integers(0, 16, shape)
            v[pick == 0] = 0.0
            v[pick == 1] = -0.0
            den = (rng.integers(1, 1 << 23, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31))
            v[pick == 2] = den.view(np.float32)[pick == 2]   # denormals of either sign
        out[name] = np.ascontiguousarray(v)
    return out


def reference(slots, grads):
    """-> (ref float64 [20,256], abs-sum float64 [20,256], member count int64 [20,256]) over the slot rows."""
    centre = slots[:, 0] * 256 + slots[:, 1]
    flat = [grads[n].reshape(-1).astype(np.float64) if grads[n] is not None else None for n in TENSORS]
    v = np.zeros(len(slots), np.float64)
    for t in range(5):
        sel = slots[:, 2] == t
        if flat[t] is not None:
            v[sel] = flat[t][slots[sel, 3]]
    ref, mag = np.zeros(5120), np.zeros(5120)
    np.add.at(ref, centre, v)
    np.add.at(mag, centre, np.abs(v))
    return ref.reshape(20, 256), mag.reshape(20, 256), np.bincount(centre, minlength=5120).reshape(20, 256)


def bar(ref, mag, n):
    """|got - ref| <= 2^-24 |ref| + n 2^-52 sum|v_i| + 2^-149: double accumulation (n additions of relative error 2^-53
    each, twice over for the reference's own sum), one rounding to float (2^-24 relative, 2^-149 among the denormals)."""
    return 2.0 ** -24 * np.abs(ref) + n * 2.0 ** -52 * mag + 2.0 ** -149


def check(got, slots, grads, what=""):
    ref, mag, n = reference(slots, grads)
    got = np.asarray(got).reshape(20, 256)
    assert got.dtype == np.float32
    err, lim = np.abs(got.astype(np.float64) - ref), bar(ref, mag, n)
    worst = np.unravel_index(np.argmax(err - lim), err.shape)
    print(f"{what}: worst centre {worst}: err {err[worst]:.3e} bar {lim[worst]:.3e} (n {n[worst]})")
    assert (err <= lim).all(), (what, worst, err[worst], lim[worst])
    assert (got.view(np.uint32)[n == 0] == 0).all(), (what, "a centre without a member must be +0.0")
