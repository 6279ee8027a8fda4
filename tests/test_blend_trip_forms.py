"""The per-lane functions of one (entry, quadrant) trip of the blend kernels (blend_math.h: fwd_alpha, fwd_apply, bwd_test,
bwd_accumulate, splat_grad_of) in the form before the trip was rewritten (-DR3_OLD_TRIP_FORMS) and in today's form, run on
the CPU over a seeded sweep and compared BIT FOR BIT.  Both builds have FMA contraction on, as blend.hip has on the GPU, so
that the old form's  T - alpha T  is contracted by the compiler the way the device compiler contracts it and the new form's
explicit fma has to reproduce it.  The sweep contains alpha exactly at 1/255 and at 0.99, T at 1e-4, power at +0 and -0,
sums that start at -0.0, and NaN / inf conics.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.hostcheck_build import build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_trip", "hostcheck_trip.hip")


def _cpu_has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read().replace("\n", " ")
    except OSError:
        return False


def _lib(old):
    so = os.path.join(HERE, "hostcheck_trip", f"libtrip_{'old' if old else 'new'}.so")
    return build_shim(SRC, so, ["-ffp-contract=fast", "-mfma"] + (["-DR3_OLD_TRIP_FORMS"] if old else []), None)


def _sweep():
    rng = np.random.default_rng(20240611)
    n = 20000
    f32 = np.float32
    v = np.zeros((n, 16), f32)
    v[:, 0:2] = rng.uniform(0, 64, (n, 2))                       # mean
    a, c = rng.uniform(0.01, 4.0, (2, n))
    b = rng.uniform(-1, 1, n) * np.sqrt(a * c)
    v[:, 2], v[:, 3], v[:, 4] = -0.5 * 1.4426950408889634 * a, -1.4426950408889634 * b, -0.5 * 1.4426950408889634 * c
    v[:, 5] = rng.uniform(0.001, 1.0, n)                          # opacity
    v[:, 6:9] = rng.uniform(0, 1, (n, 3))                         # colour
    v[:, 9:11] = np.floor(v[:, 0:2] + rng.uniform(-2, 2, (n, 2)))  # pixel, within reach of the splat
    v[:, 11] = rng.uniform(0, 1, n) ** 4                          # T, many small
    v[:, 12] = rng.normal(0, 1, n)                                # A
    v[:, 13:16] = rng.normal(0, 1, (n, 3))                        # dL/dpixel
    aux = np.zeros((n, 3), np.uint32)
    aux[:, 0] = rng.integers(0, 100, n)
    aux[:, 1] = rng.integers(0, 100, n)
    aux[:, 2] = np.where(rng.random(n) < 0.5, 0x80000000, 0)      # sums start at -0.0 or +0.0
    # --- the edges, on the first rows: pixel == mean so that power is a signed zero and alpha == opacity exactly
    k = 0
    one255 = f32(1.0) / f32(255.0)
    edges_op = [one255, np.nextafter(one255, f32(0)), np.nextafter(one255, f32(1)), f32(0.99), np.nextafter(f32(0.99), f32(0)),
                np.nextafter(f32(0.99), f32(1)), f32(1.0), f32(0.5)]
    edges_T = [f32(1e-4), np.nextafter(f32(1e-4), f32(0)), np.nextafter(f32(1e-4), f32(1)), f32(1.0), f32(0.0), f32(-1.0),
               f32(1e-4) / (f32(1) - one255), f32(1.0001e-4)]
    for op in edges_op:
        for T in edges_T:
            for sign in (1.0, -1.0):                              # conic signs: power = -0.0 or +0.0
                for last in (0, 5, 6):
                    v[k, 0:2] = v[k, 9:11]
                    v[k, 2:5] *= sign
                    v[k, 5], v[k, 11] = op, T
                    aux[k, 0], aux[k, 1] = 5, last
                    k += 1
    for bad in (np.nan, np.inf, -np.inf, 0.0):                    # NaN / inf / zero conics and opacities, on and off the mean
        for col in (2, 3, 4, 5):
            for on_mean in (True, False):
                v[k, col] = bad
                if on_mean:
                    v[k, 0:2] = v[k, 9:11]
                aux[k, 0], aux[k, 1] = 3, 9
                k += 1
    assert k < 1000
    return np.ascontiguousarray(v), np.ascontiguousarray(aux)


NAMES = (["fwd alpha", "fwd in_bound", "fwd result", "fwd T", "fwd Tf", "fwd C0", "fwd C1", "fwd C2", "fwd last", "fwd T_before",
          "fwd live", "bwd valid", "bwd in_list", "bwd in_bound", "bwd visible", "bwd G", "bwd alpha", "bwd T", "bwd A"] +
         ["sum " + c for c in "sx sy sxx sxy syy sm r g b".split()] + ["grad " + c for c in "mx my cA cB cC op r g b".split()] +
         ["dxx", "dxy", "dyy"])


def test_trip_forms_old_and_new_agree_bit_for_bit():
    if not _cpu_has_fma():
        pytest.fail("this CPU has no FMA instruction: the contracted forms of blend.hip cannot be reproduced on it")
    v, aux = _sweep()
    outs = []
    for old in (True, False):
        out = np.zeros((len(v), 40), np.uint32)
        _lib(old).trip_sweep(C.c_int(len(v)), v.ctypes.data_as(C.c_void_p), aux.ctypes.data_as(C.c_void_p),
                             out.ctypes.data_as(C.c_void_p))
        outs.append(out)
    old, new = outs
    # the sweep does reach the branches it is meant to reach
    assert {0, 1, 2} <= set(new[:, 2].tolist()) and new[:, 11].sum() > 1000 and (new[:, 11] == 0).sum() > 1000
    assert np.isnan(new[:, 0].view(np.float32)).any() or np.isnan(new[:, 15].view(np.float32)).any()
    diff = np.argwhere(old != new)
    assert len(diff) == 0, "first differences (row, field): " + ", ".join(
        f"({r}, {NAMES[c]}: {old[r, c]:#x} != {new[r, c]:#x})" for r, c in diff[:8])
