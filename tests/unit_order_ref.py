"""The rule of the backward blend's unit order (reduced-3dgs_amd/csrc/unit_order.h, common.h TileGrid) restated in numpy, and
the host shim that replays the header itself on the CPU (tests/hostcheck_unit_order).  tests/test_unit_order_cpu.py holds the
two against each other; tests/test_gpu_parity.py holds the device's order against both."""
import ctypes as C
import os

import numpy as np

from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_unit_order", "hostcheck_unit_order.hip")
SO = os.path.join(HERE, "hostcheck_unit_order", "libhostcheck_unit_order.so")
SEG_MAX = 32      # common.h kBwdSegMax
CLASSES = 1024    # unit_order.h kOrderClasses


def unit_list_tiles(g_, gx, gy, block=4, lists=8):
    """Tiles of unit list g_ of the backward blend (common.h TileGrid): the block x block tile blocks g_, g_ + lists, ... of
    the image (blocks row-major, tiles row-major inside a block, tiles outside the image left out)."""
    bx, by = (gx + block - 1) // block, (gy + block - 1) // block
    out = []
    for k in range(g_, bx * by, lists):
        for o in range(block * block):
            tx, ty = k % bx * block + o % block, k // bx * block + o // block
            if tx < gx and ty < gy:
                out.append(ty * gx + tx)
    return np.array(out, np.int64)


def unit_list_fit(pairs, gx, gy, block=4, lists=8):
    """Units a list may hold in a pass of `pairs` pairs (common.h bwd_list_fit)."""
    bx, by = (gx + block - 1) // block, (gy + block - 1) // block
    return min((bx * by + lists - 1) // lists * block * block, gx * gy) + min(pairs >> 7, 8 * gx * gy) // lists


def tile_segments(length, qd, thr, walk):
    """Units of each tile whose list is `length` long and whose quadrants' deepest contributors are qd[:, 4], walked in
    segments of `walk` entries (0: whole tiles): lists of at least `thr` entries deeper than one segment are split into
    ceil(deepest / walk) segments, SEG_MAX at most; a tile nothing contributed to has no unit."""
    deepest = qd.max(axis=1)
    n = np.ones(len(length), np.int64)
    if walk:
        n = np.where((length >= thr) & (deepest > walk), np.minimum((deepest + walk - 1) // walk, SEG_MAX), 1)
    n[qd.sum(axis=1) == 0] = 0
    return n


def tile_full_segments(qd, n, walk):
    """Leading segments of each tile (of n units) that all four quadrants walk in full: min quadrant depth // walk, but never the
    last segment of a tile capped at SEG_MAX (it takes the rest); none for an unsplit tile."""
    if not walk:
        return np.zeros(len(n), np.int64)
    f = np.minimum(qd.min(axis=1) // walk, np.where(n == SEG_MAX, n - 1, n))
    return np.where(n > 1, f, 0)


def list_segments(length, qd, thr, fit, S=128, walks=4):
    """(walk, units per tile) of a list: the shortest of the segment lengths S, 2 S, ... whose units fit the list's slots;
    walk = 0 -- whole tiles -- if none does or the pass has no segments (S = 0)."""
    for k in range(walks if S else 0):
        n = tile_segments(length, qd, thr, S << k)
        if n.sum() <= fit:
            return S << k, n
    return 0, tile_segments(length, qd, thr, 0)


def unit_weights(qd, segment, segments, walk):
    """Entries each unit (rows of qd: its tile's quadrant depths) visits: per quadrant its depth clamped to the segment, the
    last segment of a tile taking whatever is left; an unsplit tile: the sum of its quadrants' depths."""
    lo = segment * walk
    hi = np.where(segment + 1 < segments, lo + walk, 1 << 40)
    weight = (np.clip(qd, lo[:, None], hi[:, None]) - lo[:, None]).sum(axis=1)
    weight[segments == 1] = qd.sum(axis=1)[segments == 1]
    return weight


def split_bound(walk, thr):
    """The heaviest unit of a splitting pass, known without looking: a segment weighs at most 4 x its length, an unsplit tile
    is shorter than thr entries; a capped tile's last segment may exceed it."""
    return max(4 * walk, 4 * thr)


def weight_classes(weight, heaviest):
    """The kernel's 1024 classes of a weight given the heaviest (larger = heavier; the kernel numbers them the other way
    round: class 0 the heaviest)."""
    return np.minimum((weight.astype(np.float64) * (CLASSES - 1.0) / heaviest).astype(np.int64), CLASSES - 1)


def shim():
    """The host shim (built on first use); a missing hipcc is an error, not a skip."""
    lib = build_shim(SRC, SO, EXACT, None)
    lib.hu_pack.restype = C.c_uint
    lib.hu_addressing.restype = C.c_uint
    lib.hu_replay.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def replay(lib, gx, gy, list_, quad_depth, ranges, num_pairs, seg_log2, thr):
    """unit_order.h's own order of one list: dict(words, weight, klass -- the kernel's numbering, 0 the heaviest --, full -- per
    tile of the image, the full segments of the list's tiles --, units, walk_log2); units in class order, ties in slot order."""
    qd = np.ascontiguousarray(quad_depth, np.uint32).reshape(gx * gy, 4)
    rg = np.ascontiguousarray(ranges, np.uint32).reshape(gx * gy, 2)
    cap = (SEG_MAX + 1) * (gx * gy + 16)
    words, weight, klass = (np.zeros(cap, np.uint32) for _ in range(3))
    trailer, full = np.zeros(2, np.uint32), np.zeros(gx * gy, np.uint32)
    n = lib.hu_replay(int(gx), int(gy), int(list_), _p(qd), _p(rg), C.c_uint(int(num_pairs)), C.c_uint(int(seg_log2)),
                      C.c_uint(int(thr)), _p(words), _p(weight), _p(klass), _p(full), cap, _p(trailer))
    assert n >= 0 and n == int(trailer[0])
    return dict(words=words[:n].astype(np.int64), weight=weight[:n].astype(np.int64), klass=klass[:n].astype(np.int64),
                full=full.astype(np.int64), units=n, walk_log2=int(trailer[1]))
