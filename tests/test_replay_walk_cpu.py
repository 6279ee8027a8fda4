"""CPU checks of the replay passes' index arithmetic (reduced-3dgs_amd/csrc/replay_walk.h): the header's own xcd_remap,
quad_lane and walk_span, called through tests/hostcheck_walk, against plain Python, and of the host plan of a replay backward
(pass_driver.h replay_bwd_plan).  No GPU needed."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from tests.hostcheck_build import EXACT, HIPCC, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_walk", "hostcheck_walk.hip")
SO = os.path.join(HERE, "hostcheck_walk", "libhostcheck_walk.so")
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    lib = build_shim(SRC, SO, EXACT, None)
    lib.hw_xcd_remap.restype = C.c_uint
    lib.hw_xcd_remap.argtypes = [C.c_uint, C.c_uint]
    lib.hw_quad_lane.restype = None
    lib.hw_quad_lane.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.hw_walk_span.restype = None
    lib.hw_walk_span.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(C.c_uint)]
    lib.hw_replay_bwd_plan.restype = C.c_int
    lib.hw_replay_bwd_plan.argtypes = [C.c_int] * 4
    return lib


NBLOCKS = sorted(set(range(1, 71)) | {8 * k + d for k in range(1, 513) for d in (-1, 1) if 8 * k + d <= 4099})


def test_xcd_remap_is_a_permutation(lib):
    assert NBLOCKS[-1] == 4097 and 4095 in NBLOCKS
    for n in NBLOCKS:
        got = sorted(lib.hw_xcd_remap(b, n) for b in range(n))
        assert got == list(range(n)), n
    # a multiple of 8: block b runs on XCD b % 8, and logical ids are consecutive there
    assert [lib.hw_xcd_remap(b, 16) for b in range(16)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]


@pytest.mark.parametrize("W,H", [(17, 9), (33, 17)])
def test_quad_lane_covers_every_pixel_once(lib, W, H):
    tile = lib.hw_tile()
    gx, gy = (W + tile - 1) // tile, (H + tile - 1) // tile
    seen = {}
    out = (C.c_longlong * 10)()
    for wg, lane in itertools.product(range(gx * gy * 4), range(64)):
        lib.hw_quad_lane(wg, lane, gx, W, H, out)
        t, quad, px, py, inside, pix, qx0, qy0, pxf, pyf = list(out)
        assert (t, quad) == (wg // 4, wg % 4)
        # the quadrant's corner and the lane's pixel in it, in plain Python
        x0, y0 = (t % gx) * tile + (quad & 1) * 8, (t // gx) * tile + (quad >> 1) * 8
        assert (qx0, qy0, px, py, pxf, pyf) == (x0, y0, x0 + lane % 8, y0 + lane // 8, px, py)
        assert bool(inside) == (px < W and py < H)   # it marks no pixel outside
        if inside:
            assert pix == py * W + px
            seen[pix] = seen.get(pix, 0) + 1
    assert sorted(seen) == list(range(W * H)) and set(seen.values()) == {1}


def forward_form(rx, ry, qd, R):
    """The span as the forward walks wrote it: first / end."""
    length = ry - rx if ry > rx else 0
    length = min(length, qd)
    first = min(rx, R)
    return first, first + min(length, (R - first) & U32)


def backward_form(rx, ry, qd, R):
    """... and as the backward walks wrote it: first / list_len / len."""
    full = ry - rx if ry > rx else 0
    first = min(rx, R)
    list_len = min(full, (R - first) & U32)
    return first, list_len, min(list_len, qd)


def span_cases():
    for R in (1, 64, 200):
        for rx in (0, R - 1, R, R + 5):
            ys = {rx - 1, rx, rx + 1, rx + 63, R - 1, R, R + 1, R + 70, 3 * R + 100}   # below, equal to, above rx; around and above R
            for ry in sorted(y for y in ys if y >= 0):
                for qd in (0, 1, 63, 64, 65, U32):
                    yield rx, ry, qd, R


def test_walk_span(lib):
    out = (C.c_uint * 3)()
    cut = 0
    for rx, ry, qd, R in span_cases():
        lib.hw_walk_span(rx, ry, qd, R, out)
        first, list_len, length = list(out)
        case = (rx, ry, qd, R)
        assert first + list_len <= R, case          # the list inside the blob: fails without `R - first` in the clamp
        assert length <= list_len, case
        assert length <= qd, case
        assert (first, list_len, length) == backward_form(rx, ry, qd, R), case
        assert (first, first + length) == forward_form(rx, ry, qd, R), case
        cut += ry > R and ry > rx
    assert cut > 50   # the cases do reach lists that run past the blob


NOTHING, ZERO_OUTPUTS, WALK = 0, 1, 2


def plan_cases():
    """(P, R, upstream, outputs) -> the plan: DESIGN.md's contract written out row by row, no expression shared with the code."""
    N, Z, W = NOTHING, ZERO_OUTPUTS, WALK
    return {
        (0, 0, 0, 0): N, (0, 0, 0, 1): N, (0, 0, 1, 0): N, (0, 0, 1, 1): N,   # P == 0: every output has P rows
        (0, 1, 0, 0): N, (0, 1, 0, 1): N, (0, 1, 1, 0): N, (0, 1, 1, 1): N,
        (1, 0, 0, 0): Z, (1, 0, 0, 1): Z, (1, 0, 1, 0): Z, (1, 0, 1, 1): Z,   # R == 0: nothing to walk, asked for or not
        (1, 1, 0, 0): Z, (1, 1, 0, 1): Z,                                     # no upstream: the same
        (1, 1, 1, 0): N,                                                      # pairs and an upstream, but nothing asked for
        (1, 1, 1, 1): W,
    }


def test_replay_bwd_plan_truth_table(lib):
    table = plan_cases()
    assert len(table) == 16 and sorted(set(table.values())) == [NOTHING, ZERO_OUTPUTS, WALK]
    assert table[1, 1, 1, 1] == WALK and sum(v == WALK for v in table.values()) == 1
    assert table[1, 0, 1, 0] == ZERO_OUTPUTS and table[1, 1, 0, 0] == ZERO_OUTPUTS   # "nothing to walk" before "nothing asked"
    for case, want in table.items():
        assert lib.hw_replay_bwd_plan(*case) == want, case


SAN = ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined")


@pytest.mark.parametrize("name,extra", [("hostcheck_walk", ()), ("hostcheck_walk_san", SAN)])
def test_replay_bwd_plan_program(name, extra):
    """The same table checked by the stand-alone program, plainly and under the host sanitizers."""
    exe = os.path.join(HERE, "hostcheck_walk", name)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", *EXACT, *extra, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    rows = out.stdout.split()
    table = plan_cases()
    assert len(rows) == 16 * 5
    for k in range(16):
        P, R, up, outs, plan = (int(f.split("=")[1]) for f in rows[5 * k:5 * k + 5])
        assert table[P, R, up, outs] == plan
