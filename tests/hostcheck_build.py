"""The one recipe of the host-check shims: a tests/hostcheck*/*.hip file that includes the product's __host__ __device__
headers is compiled by hipcc into a shared library next to it and loaded with ctypes, so that the arithmetic a lane executes
runs on the CPU.  A shim is rebuilt when its source or ANY header under reduced-3dgs_amd/csrc/ or include/ is newer than it
(the rule of reduced-3dgs_amd/build.py: no hand-kept header lists)."""
import ctypes
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# no contraction, correctly rounded fp32 divide and sqrt: the flags of the product's bit-exact translation units
EXACT = ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt")


def _headers():
    return glob.glob(os.path.join(ROOT, "reduced-3dgs_amd", "csrc", "*.h")) + glob.glob(os.path.join(ROOT, "include", "*.h"))


def build_shim(src, so, flags, skip):
    """Compiles `src` to `so` with hipcc and the extra `flags` if `so` is missing or stale, and returns ctypes.CDLL(so).
    Without hipcc: pytest.skip(skip), or an assertion failure when `skip` is None (a test that must not skip)."""
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + _headers()):
        if skip is None:
            assert os.path.exists(HIPCC), "hipcc is needed to build the host shim"
        elif not os.path.exists(HIPCC):
            pytest.skip(skip)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-o", so, src])
    return ctypes.CDLL(so)
