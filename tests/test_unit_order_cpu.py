"""CPU checks of the backward blend's unit order (reduced-3dgs_amd/csrc/unit_order.h): the header's own functions, replayed
serially by tests/hostcheck_unit_order, against the numpy statement of the rule in tests/unit_order_ref.py, on synthetic
quadrant depths and list lengths that reach every branch of the rule.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import unit_order_ref as ref

S_LOG2, S, THR = 7, 128, 300
GRIDS = [(1, 1), (5, 3), (33, 9), (129, 2)]   # one tile; edge blocks with tile-less slots; more blocks than lists;
                                              # list_slots above list_tiles_max


@pytest.fixture(scope="module")
def lib():
    return ref.shim()


@pytest.fixture(scope="module")
def fields():
    from diff_gaussian_rasterization import _C
    return _C.unit_fields


# (list length, quadrant depths) of the per-tile cases
TILE_CASES = [
    (500, (0, 0, 0, 0)),                               # nothing contributed: no unit
    (THR - 1, (1000, 900, 800, 700)),                  # one entry too short for checkpoints: one unit however deep
    (THR, (300, 290, 280, 270)),                       # just long enough: split
    (2000, (S, S - 1, 5, 0)),                          # deepest contributor S: one segment holds it
    (2000, (S + 1, S, 5, 1)),                          # S + 1: two
    (2000, (0, 700, 700, 650)),                        # one quadrant empty: no segment is walked in full by all four
    (6000, (32 * S + 900, 32 * S + 800, 4500, 3000)),  # deeper than 32 S: capped, the last segment takes the rest
    (2000, (1000, 1000, 1000, 1000)),                  # every segment full but the last (deepest is no multiple of S)
    (2000, (1024, 1024, 1024, 1024)),                  # every segment full
    (6000, (32 * S + 900,) * 4),                       # capped and every quadrant deeper than 32 S: all full but the last
]
SEGMENTS_AT_S = [0, 1, 3, 1, 2, 6, 32, 8, 8, 32]   # units of each case walked in segments of S, and how many of them are full
FULL_AT_S = [0, 0, 2, 0, 0, 0, 23, 7, 8, 31]


def scene(gx, gy, rotation):
    """Tile t of the grid gets case (t + rotation) % cases; the lists lie behind one another as the binning leaves them."""
    Tn = gx * gy
    pick = (np.arange(Tn) + rotation) % len(TILE_CASES)
    length = np.array([TILE_CASES[k][0] for k in pick], np.int64)
    qd = np.array([TILE_CASES[k][1] for k in pick], np.int64).reshape(Tn, 4)
    first = np.concatenate([[0], np.cumsum(length)[:-1]])
    return qd, np.stack([first, first + length], axis=1)


def check_list(lib, fields, gx, gy, g_, qd, ranges, pairs, seg_log2=S_LOG2, thr=THR):
    """Every property of one list's replayed order; returns (walk, replay)."""
    rep = ref.replay(lib, gx, gy, g_, qd, ranges, pairs, seg_log2, thr)
    mine = ref.unit_list_tiles(g_, gx, gy)
    length = ranges[:, 1] - ranges[:, 0]
    fit = ref.unit_list_fit(pairs, gx, gy)
    walk, n_g = ref.list_segments(length[mine], qd[mine], thr, fit, (1 << seg_log2) if seg_log2 else 0)
    # the trailer: the list's units and the segment length they walk; never more units than the list may launch
    assert rep["walk_log2"] == (walk.bit_length() - 1 if walk else 0)
    assert rep["units"] == n_g.sum() <= fit
    # _C.py's masks read the header's words as the header does
    u = fields(rep["words"])
    out = np.zeros(3, np.uint32)
    for w, t, k, n in zip(rep["words"], u["tile"], u["segment"], u["segments"]):
        lib.hu_unpack(C.c_uint(int(w)), out.ctypes.data_as(C.c_void_p))
        assert (int(t), int(k), int(n)) == tuple(int(v) for v in out) and lib.hu_pack(int(t), int(k), int(n)) == int(w)
    # every (tile, segment) of the list's tiles exactly once, each with its tile's segment count
    want = np.concatenate([[t * 64 + k for k in range(n)] for t, n in zip(mine, n_g) if n] or [[]]).astype(np.int64)
    assert np.array_equal(np.sort(u["tile"] * 64 + u["segment"]), np.sort(want))
    n_want = np.zeros(gx * gy, np.int64)
    n_want[mine] = n_g
    assert np.array_equal(u["segments"], n_want[u["tile"]])
    # weights; classes heaviest first (the kernel's class 0 is the heaviest) and the reference's up to the fp32 product
    weight = ref.unit_weights(qd[u["tile"]], u["segment"], u["segments"], walk)
    assert np.array_equal(rep["weight"], weight)
    # the header's full segments: the numpy count per tile, and each of them weighs 4 x the segment length (which is why the
    # kernel may give them that weight's class without looking)
    full = np.zeros(gx * gy, np.int64)
    full[mine] = ref.tile_full_segments(qd[mine], n_g, walk)
    assert np.array_equal(rep["full"], full)
    assert np.all(weight[u["segment"] < full[u["tile"]]] == 4 * walk)
    assert np.all(np.diff(rep["klass"]) >= 0)
    heaviest = ref.split_bound(walk, thr) if walk else max(int(qd[mine].sum(axis=1).max()) if len(mine) else 0, 1)
    assert np.all(np.abs((ref.CLASSES - 1 - ref.weight_classes(weight, heaviest)) - rep["klass"]) <= 1)
    # ties inside a class: slot order, a tile's segments ascending
    pos = np.zeros(gx * gy, np.int64)
    pos[mine] = np.arange(len(mine))
    key = pos[u["tile"]] * 64 + u["segment"]
    assert np.all((np.diff(rep["klass"]) > 0) | (np.diff(key) > 0))
    return walk, rep


def test_word_format_and_list_addressing(lib, fields):
    consts = np.zeros(6, np.int32)
    lib.hu_constants(consts.ctypes.data_as(C.c_void_p))
    lists, classes, walks, seg_max, tile_bits, seg_bits = (int(v) for v in consts)
    assert (lists, classes, walks, seg_max) == (8, ref.CLASSES, 4, ref.SEG_MAX)
    assert seg_max < 1 << seg_bits and tile_bits + 2 * seg_bits <= 32
    rng = np.random.default_rng(0)
    for t, k, n in [(0, 0, 1), ((1 << tile_bits) - 1, seg_max - 1, seg_max), (12345, 7, 9)] + [
            (int(rng.integers(1 << tile_bits)), int(rng.integers(seg_max)), int(rng.integers(1, seg_max + 1))) for _ in range(200)]:
        w = lib.hu_pack(t, k, n)
        assert w == t | k << tile_bits | n << (tile_bits + seg_bits)
        f = fields(np.array([w], np.int64))
        assert (int(f["tile"][0]), int(f["segment"][0]), int(f["segments"][0])) == (t, k, n)
    # what _C.export_tile_order reads: lists of cap / 8 slots, behind them one {units, walk_log2} pair per list
    info = np.zeros(3, np.uint32)
    for cap in (8, 64, 8 * 1201):
        for g_ in range(lists):
            assert lib.hu_addressing(cap, g_, info.ctypes.data_as(C.c_void_p)) == cap + 2 * lists
            assert tuple(int(v) for v in info) == (cap // lists, g_ * (cap // lists), cap + 2 * g_)


@pytest.mark.parametrize("gx,gy", GRIDS)
def test_every_tile_case_on_every_grid(lib, fields, gx, gy):
    Tn = gx * gy
    seen_walks = set()
    for rotation in range(len(TILE_CASES)):
        qd, ranges = scene(gx, gy, rotation)
        for pairs in (0, Tn << 7, (8 * Tn) << 7):
            for g_ in range(8):
                walk, rep = check_list(lib, fields, gx, gy, g_, qd, ranges, pairs)
                seen_walks.add(walk)
                u = fields(rep["words"])
                if walk == S:
                    for t in np.unique(u["tile"]):
                        case = (t + rotation) % len(TILE_CASES)
                        n = int(u["segments"][u["tile"] == t][0])
                        assert n == SEGMENTS_AT_S[case] and rep["full"][t] == FULL_AT_S[case]
                        if n == 32:   # the capped tile's last segment: heavier than the bound, in the heaviest class
                            last = (u["tile"] == t) & (u["segment"] == 31)
                            assert rep["weight"][last][0] > ref.split_bound(walk, THR) and rep["klass"][last][0] == 0
        # segments off / no checkpoints: whole tiles whatever the lists
        for g_ in range(8):
            walk, rep = check_list(lib, fields, gx, gy, g_, qd, ranges, (8 * Tn) << 7, seg_log2=0)
            assert walk == 0 and np.all(fields(rep["words"])["segments"] == 1)
    assert S in seen_walks, "the shortest segments must fit somewhere on this grid"


def test_full_segments_share_the_class_of_four_segment_lengths(lib, fields):
    """What lets the kernel count and place a tile's full segments as a group: a segment all four quadrants walk in full weighs
    4 x its length and falls into one class, whichever tile it belongs to."""
    empty_q, but_last, all_full = 1, 2, 5   # tiles of list 0 of a 5 x 3 grid; every other tile has nothing
    qd = np.zeros((15, 4), np.int64)
    qd[empty_q], qd[but_last], qd[all_full] = (0, 700, 700, 650), (1000,) * 4, (1024,) * 4
    first = np.arange(15, dtype=np.int64) * 2000
    ranges = np.stack([first, first + 2000], axis=1)
    for g_ in range(8):
        walk, rep = check_list(lib, fields, 5, 3, g_, qd, ranges, (8 * 15) << 7)
        assert walk == S and rep["units"] == (6 + 8 + 8 if g_ == 0 else 0)
        u = fields(rep["words"])
        full = (u["segments"] > 1) & ((u["segment"] + 1) * walk <= qd[u["tile"]].min(axis=1))
        assert full.sum() == (7 + 8 if g_ == 0 else 0)
        if g_ == 0:
            assert (rep["full"][empty_q], rep["full"][but_last], rep["full"][all_full]) == (0, 7, 8)
        assert np.all(rep["weight"][full] == 4 * walk) and len(set(rep["klass"][full])) <= 1
        # the quadrant-empty tile has no full segment, the all-full tile has nothing else
        assert np.all(rep["weight"][u["tile"] == empty_q] < 4 * S) and np.all(rep["weight"][u["tile"] == all_full] == 4 * S)


@pytest.mark.parametrize("depth,extra,walk_want", [(300, None, S), (300, "twice", 2 * S), (3000, 0, 0)],
                         ids=["shortest_fits", "twice_the_length_fits_exactly", "none_fits_whole_tiles"])
def test_walk_is_the_shortest_that_fits(lib, fields, depth, extra, walk_want):
    """The segment length of a list is the first of S, 2 S, 4 S, 8 S whose units fit what the list may launch, else whole
    tiles.  33 x 9 tiles, every list long and `depth` deep: list 0 holds 40 tiles -- 3 units each at S and 2 at 2 S for a
    depth of 300; 3 each even at 8 S for 3000."""
    gx, gy, Tn = 33, 9, 33 * 9
    qd = np.full((Tn, 4), depth, np.int64)
    first = np.arange(Tn, dtype=np.int64) * 4000
    ranges = np.stack([first, first + 4000], axis=1)
    t0 = len(ref.unit_list_tiles(0, gx, gy))
    tiles_max = ref.unit_list_fit(0, gx, gy)
    assert (t0, tiles_max) == (40, 64)
    # pairs that give list 0 exactly the slots of its units at 2 S / every slot a pass can have / none beyond its tiles
    pairs = {None: (8 * Tn) << 7, "twice": (8 * (2 * t0 - tiles_max)) << 7, 0: 0}[extra]
    walk, rep = check_list(lib, fields, gx, gy, 0, qd, ranges, pairs)
    assert walk == walk_want
    assert rep["units"] == {S: 3 * t0, 2 * S: 2 * t0, 0: t0}[walk_want]
    if extra == "twice":
        assert rep["units"] == ref.unit_list_fit(pairs, gx, gy) < 3 * t0
    for g_ in range(1, 8):
        check_list(lib, fields, gx, gy, g_, qd, ranges, pairs)
