"""CPU checks of the visibility-gated Adam step (r3dgs_optim.Adam.step(radii=...), csrc/optim.hip's adam_visible_kernel,
include/r3dgs_optim.h): the per-lane logic the kernel calls (csrc/adam_math.h: the element-to-Gaussian mapping and the
gated element) runs on the host through a test shim.  The mapping must equal e // row_len wherever the kernel takes a
different route, and a gated step must equal the float32 restatement (tests/adam_ref.step32) on the visible rows bit for
bit and return the input bits on the others, whatever their gradients hold.  The Python surface takes keyword-only radii
and refuses what the kernel cannot take before any step count moves.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import zlib

import numpy as np
import pytest
import torch

import r3dgs_optim
from tests import adam_ref
from tests.test_optim_cpu import _bits_equal, _inputs
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_optim_rows", "hostcheck_optim_rows.hip")
SO = os.path.join(HERE, "hostcheck_optim_rows", "libhostcheck_optim_rows.so")
HEADER = os.path.join(HERE, "..", "include", "r3dgs_optim.h")
F32 = np.float32
ROW_LENS = [1, 2, 3, 4, 5, 7, 45, 48]
CHUNK_UNITS = 1024   # optim.hip: 256 threads x 4 units


def _shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the gated-step host-check shim")
    lib.hc_row_divmod.restype = C.c_uint
    lib.hc_row_divmod.argtypes = [C.c_int, C.c_uint, C.POINTER(C.c_uint)]
    lib.hc_chunk_origin.restype = C.c_longlong
    lib.hc_chunk_origin.argtypes = [C.c_int, C.c_longlong, C.POINTER(C.c_uint)]
    lib.hc_vector_row_gaussian.restype = C.c_longlong
    lib.hc_vector_row_gaussian.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong]
    lib.hc_scalar_row_gaussian.restype = C.c_longlong
    lib.hc_scalar_row_gaussian.argtypes = [C.c_int, C.c_longlong]
    lib.hc_adam_step_visible.restype = None
    lib.hc_adam_step_visible.argtypes = [C.c_int, C.c_longlong, C.c_int] + [C.c_void_p] * 6
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the mapping

@pytest.mark.parametrize("row_len", ROW_LENS + [2 ** 31 - 1])
def test_divmod_by_multiply_high(row_len):
    """row_divmod: quotient and remainder for 32-bit x, at the values where the multiply-high is one short."""
    lib = _shim()
    rng = np.random.default_rng(row_len % 1000)
    xs = {0, 1, row_len - 1, row_len, row_len + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1}
    xs |= {k * row_len + d for k in (1, 2, 1000, (2 ** 32 - 1) // row_len) for d in (-1, 0, 1)}
    xs |= set(int(x) for x in rng.integers(0, 2 ** 32, 300))
    for x in sorted(x for x in xs if 0 <= x < 2 ** 32):
        rem = C.c_uint()
        q = lib.hc_row_divmod(row_len, x, C.byref(rem))
        assert (q, rem.value) == divmod(x, row_len), (row_len, x)


@pytest.mark.parametrize("row_len", ROW_LENS)
def test_chunk_origin_below_and_above_32_bits(row_len):
    """chunk_origin as plain arithmetic, no memory: element offsets around 2^31 and 2^32 and far above."""
    lib = _shim()
    for e0 in (0, 4096, 2 ** 31 - 4, 2 ** 31, 2 ** 31 + 4096 + 3, 2 ** 32 - 4, 2 ** 32, 2 ** 32 + 4099, 3 * 2 ** 33 + 1,
               2 ** 40 + 12345):
        rem = C.c_uint()
        g = lib.hc_chunk_origin(row_len, e0, C.byref(rem))
        assert (g, rem.value) == divmod(e0, row_len), (row_len, e0)


@pytest.mark.parametrize("head", [0, 1, 2, 3])
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_vector_row_mapping(row_len, head):
    """Every element of a vector row reaches e // row_len by the kernel's route: the head, the units on either side of
    the chunk boundary (units 1023 / 1024), the tail and the last element; then the same far past 2^31 elements."""
    lib = _shim()
    P = (2 * 4 * CHUNK_UNITS + 64) // row_len + 3   # more than two chunks of float4 units
    n = P * row_len
    es = set(range(0, 40)) | set(range(n - 12, n))
    for boundary in (head + 4 * CHUNK_UNITS, head + 8 * CHUNK_UNITS):
        es |= set(range(boundary - 12, boundary + 12))
    es |= set(int(x) for x in np.random.default_rng(row_len + head).integers(0, n, 400))
    for e in sorted(e for e in es if 0 <= e < n):
        assert lib.hc_vector_row_gaussian(row_len, P, head, e) == e // row_len, (row_len, head, e)
    assert lib.hc_vector_row_gaussian(row_len, P, head, n - 1) == P - 1
    big_P = (2 ** 31 + 2 ** 29) // row_len + 5   # no memory behind it: the arithmetic only
    big_n = big_P * row_len
    for e in (2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 4 * CHUNK_UNITS + head, big_n - 5, big_n - 1):
        assert lib.hc_vector_row_gaussian(row_len, big_P, head, e) == e // row_len, (row_len, head, e)
    huge_P = (2 ** 33) // row_len + 7            # past 2^32 elements: the 64-bit division of chunk_origin
    for e in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 4097, huge_P * row_len - 1):
        assert lib.hc_vector_row_gaussian(row_len, huge_P, head, e) == e // row_len, (row_len, head, e)


@pytest.mark.parametrize("row_len", ROW_LENS)
def test_scalar_row_mapping(row_len):
    lib = _shim()
    es = set(range(0, 100)) | set(range(CHUNK_UNITS - 50, CHUNK_UNITS + 50)) | {2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1025,
                                                                                2 ** 32 + 5, 2 ** 35 + 77}
    for e in sorted(es):
        assert lib.hc_scalar_row_gaussian(row_len, e) == e // row_len, (row_len, e)


# ---- the gated element against the restatement

MASKS = ("all", "none", "alternating", "runs", "random")


def _radii(rng, P, mask):
    vis = {"all": np.ones(P, bool), "none": np.zeros(P, bool), "alternating": np.arange(P) % 2 == 0,
           "runs": (np.arange(P) // 3) % 2 == 0, "random": rng.random(P) < 0.3}[mask]
    radii = np.where(vis, rng.integers(1, 2 ** 31 - 1, P), np.where(rng.random(P) < 0.5, 0, -rng.integers(1, 2 ** 31, P)))
    return radii.astype(np.int32), vis


@pytest.mark.parametrize("kind", ["random", "zeros", "tiny_v", "huge_g"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("row_len", ROW_LENS)
def test_gated_step_matches_the_restatement_under_a_mask(row_len, mask, kind):
    """A gated step of a [P, row_len] row on the host: visible rows equal adam_ref.step32 bit for bit, invisible rows
    return their input bits although their gradients hold NaN, +Inf and -Inf."""
    lib = _shim()
    rng = np.random.default_rng(zlib.crc32(f"{row_len} {mask} {kind}".encode()))
    P = 4200 // row_len + 2
    n = P * row_len
    head = row_len % 4
    p, g, m, v = _inputs(rng, n, kind)
    radii, vis = _radii(rng, P, mask)
    vis_e = np.repeat(vis, row_len)
    g = g.copy()
    g[~vis_e] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), int((~vis_e).sum()))
    s = adam_ref.host_scalars(0.0025, 0.9, 0.999, 1e-15, 7)
    sc = np.array([s["w1"], s["beta2"], s["w2"], s["bc2_sqrt"], s["eps"], s["step_size"]], F32)
    got = [x.copy() for x in (p, m, v)]
    lib.hc_adam_step_visible(row_len, P, head, _p(radii), _p(sc), _p(g), *(_p(x) for x in got))
    ref = adam_ref.step32(p, np.where(vis_e, g, F32(0)), m, v, s)
    for name, a, r, old in zip(("p", "exp_avg", "exp_avg_sq"), got, ref, (p, m, v)):
        assert _bits_equal(a[vis_e], r[vis_e]), f"{name}: visible rows differ from step32"
        assert _bits_equal(a[~vis_e], old[~vis_e]), f"{name}: invisible rows changed"


def test_invisible_rows_keep_nan_payloads():
    """The select returns the input bits even where p, m or v themselves are NaNs with a payload."""
    lib = _shim()
    P, row_len = 64, 3
    n = P * row_len
    bits = (np.arange(n, dtype=np.uint32) + np.uint32(0x7fa00001))
    p, m, v = bits.view(F32).copy(), (bits + np.uint32(0x1000)).view(F32).copy(), (bits ^ np.uint32(0x80000000)).view(F32).copy()
    g = np.full(n, np.nan, F32)
    radii = np.zeros(P, np.int32)
    radii[::5] = 3
    sc = np.array([0.1, 0.999, 0.001, 0.5, 1e-15, -0.01], F32)
    got = [x.copy() for x in (p, m, v)]
    lib.hc_adam_step_visible(row_len, P, 1, _p(radii), _p(sc), _p(g), *(_p(x) for x in got))
    inv = np.repeat(radii <= 0, row_len)
    for a, old in zip(got, (p, m, v)):
        assert np.array_equal(a.view(np.uint32)[inv], old.view(np.uint32)[inv])


# ---- the surface

def test_step_signature_has_keyword_only_radii():
    params = inspect.signature(r3dgs_optim.Adam.step).parameters
    assert list(params) == ["self", "closure", "radii"]
    assert params["radii"].kind is inspect.Parameter.KEYWORD_ONLY and params["radii"].default is None
    assert params["closure"].default is None
    assert "radii" in r3dgs_optim.__doc__ and "SparseAdam" in r3dgs_optim.__doc__


def test_header_declares_the_two_entry_points():
    text = open(HEADER).read()
    for name, seg in (("r3dgs_adam_step_visible", "r3dgs_adam_segment"),
                      ("r3dgs_adam_step_capturable_visible", "r3dgs_adam_capturable_segment")):
        pat = (rf"int\s+{name}\s*\(\s*int\s+n_segments\s*,\s*const\s+{seg}\s*\*\s*segments\s*,\s*const\s+int\s*\*\s*row_len\s*,"
               rf"\s*const\s+int\s*\*\s*radii\s*,\s*long\s+long\s+P\s*,\s*void\s*\*\s*stream\s*\)\s*;")
        assert re.search(pat, text), name


def _optimizer(P=6, odd=None):
    """The six groups on the host, every one with a gradient and a state at step 7; `odd`: one group given P + 1 rows."""
    params = [torch.nn.Parameter(torch.randn((P + (1 if name == odd else 0),) + shape)) for name, shape, _ in adam_ref.GROUPS]
    opt = r3dgs_optim.Adam([{"params": [p], "lr": lr, "name": name} for p, (name, _, lr) in zip(params, adam_ref.GROUPS)],
                           lr=0.0, eps=1e-15)
    for p in params:
        p.grad = torch.ones_like(p)
        opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    return params, opt


@pytest.mark.parametrize("radii,odd,exc,match", [
    (lambda P: torch.ones(P, dtype=torch.int64), None, RuntimeError, r"radii is torch\.int64.*int32"),
    (lambda P: torch.ones(P, dtype=torch.bool), None, RuntimeError, r"radii is torch\.bool.*int32"),
    (lambda P: torch.ones(P, dtype=torch.float32), None, RuntimeError, r"radii is torch\.float32.*int32"),
    (lambda P: torch.ones((P, 1), dtype=torch.int32), None, RuntimeError, r"radii has shape \(6, 1\).*1-d"),
    (lambda P: torch.ones((), dtype=torch.int32), None, RuntimeError, r"radii has shape \(\).*1-d"),
    (lambda P: torch.ones(2 * P, dtype=torch.int32)[::2], None, RuntimeError, "radii is not contiguous"),
    (lambda P: torch.ones(P, dtype=torch.int32), None, RuntimeError, "radii is a host tensor"),
    (lambda P: torch.ones(P + 2, dtype=torch.int32), None, RuntimeError,
     r"parameter 0 of group 0 \('xyz'\) has shape \(6, 3\), but radii has 8 rows"),
    (lambda P: torch.ones(P, dtype=torch.int32), "f_rest", RuntimeError,
     r"parameter 0 of group 2 \('f_rest'\) has shape \(7, 15, 3\), but radii has 6 rows"),
    (lambda P: [1] * P, None, TypeError, "radii is a list"),
])
def test_refused_radii(radii, odd, exc, match):
    """Each refusal names its offender and comes before any step count is bumped or any state is made."""
    params, opt = _optimizer(odd=odd)
    with pytest.raises(exc, match=match):
        opt.step(radii=radii(6))
    for p in params:
        assert opt.state[p]["step"].item() == 7.0
        assert not opt.state[p]["exp_avg"].any()
    fresh = torch.nn.Parameter(torch.zeros(4, 3))
    fresh.grad = torch.ones(4, 3)
    opt2 = r3dgs_optim.Adam([fresh])
    with pytest.raises(RuntimeError, match="radii is a host tensor"):
        opt2.step(radii=torch.ones(4, dtype=torch.int32))
    assert len(opt2.state) == 0


def test_parameters_without_a_gradient_are_not_checked_against_radii():
    """A parameter with no gradient takes no part in the step, so its shape is not held to radii."""
    a, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(9))
    a.grad = torch.ones(4, 3)
    opt = r3dgs_optim.Adam([a, b])
    with pytest.raises(RuntimeError, match="radii is a host tensor"):   # b's shape passed: the next refusal is reached
        opt.step(radii=torch.ones(4, dtype=torch.int32))


def test_step_without_radii_is_unchanged_on_the_host():
    """radii=None is the old path: a host parameter is still refused by the dense step's own message."""
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="host tensor"):
        r3dgs_optim.Adam([p]).step(radii=None)


# ---- the C ABI's own refusals: each comes before anything is launched, so none needs a device

def _abi_call(capturable, n, row_len, P, radii=True, step=True):
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    arrays = [np.zeros(max(n, 1), F32) for _ in range(4)]
    rad = np.ones(max(P, 1), np.int32)
    count = np.zeros(1, F32)
    ptrs = [a.ctypes.data for a in arrays]
    if capturable:
        segs = (_C._AdamCapturableSegment * 1)(_C._AdamCapturableSegment(*ptrs, count.ctypes.data if step else None, None, n,
                                                                         1e-3, 0.9, 0.999, 1e-8))
        fn = lib.r3dgs_adam_step_capturable_visible
    else:
        segs = (_C._AdamSegment * 1)(_C._AdamSegment(*ptrs, n, 0.1, 0.999, 0.001, 1.0, 1e-8, -1e-3))
        fn = lib.r3dgs_adam_step_visible
    rc = fn(1, segs, (C.c_int * 1)(row_len), rad.ctypes.data if radii else None, P, None)
    assert all(not a.any() for a in arrays) and count[0] == 0
    return rc, lib.r3dgs_last_error().decode()


@pytest.mark.parametrize("capturable", [False, True], ids=["plain", "capturable"])
def test_c_abi_refusals(capturable):
    rc, msg = _abi_call(capturable, 12, 0, 4)
    assert rc < 0 and "segment 0" in msg and "row_len 0 < 1" in msg
    rc, msg = _abi_call(capturable, 12, -3, -4)
    assert rc < 0
    rc, msg = _abi_call(capturable, 12, 3, 5)
    assert rc < 0 and "segment 0" in msg and "n 12 is not P * row_len = 5 * 3" in msg
    rc, msg = _abi_call(capturable, 12, 3, 4, radii=False)
    assert rc < 0 and "radii is NULL" in msg
    if capturable:   # what the dense call refuses is refused here too
        rc, msg = _abi_call(capturable, 12, 3, 4, step=False)
        assert rc < 0 and "step is NULL" in msg
