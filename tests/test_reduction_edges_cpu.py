"""What tests/test_reduction_edges_gpu.py rests on, checked without a GPU: the coverage claims of tests/reduction_cases.py
(from the index arithmetic and the oracle alone) and the oracle's own edge rules.
  * every position a run of intersection_kernel can take occurs in the case set; a run cut twice and knn == 0 occur;
  * the ambiguity cap and the both-outcomes condition hold on the oracle for every case;
  * the neighbour sentinel rule of include/r3dgs_reduction.h in oracle/reduction_ops.py;
  * the identity-matrix border table has an exactly-on and a just-outside point for each of the six frustum comparisons;
  * non-finite positions and NaN lengths in the oracle (the fminf rule);
  * the bfloat16 table against torch's conversion, every rounding situation in both halves of a word;
  * the region borders of the shard cases."""
import numpy as np
import pytest

from oracle import reduction_ops as ro
from tests import reduction_cases as rc

F = np.float32


# ---------------------------------------------------------------------------------------------- redundancy chain
def test_case_set_reaches_every_run_position():
    found = set()
    for P, knn in rc.CHAIN_SHAPES:
        found |= rc.run_positions(P, knn)
    assert found == set(rc.POSITIONS)
    # the issue's shapes, all of them
    for knn in rc.KNNS:
        for P in rc.SMALL_P:
            assert ((P, knn) in rc.CHAIN_SHAPES) == (P > knn)
    for knn in (127, 128, 129, 200):
        big = [P for P, k in rc.CHAIN_SHAPES if k == knn and P > 257]
        assert len(big) == 1 and big[0] <= 2000
        # with the larger P every position a run of this length can take occurs: no run of > 64 pairs is `whole`, and
        # runs of exactly two waves stay aligned (a wave's worth at the tail, one at the head, no dead lanes)
        can = {"tail", "head", "dead_block"} if knn == 128 else set(rc.POSITIONS) - {"whole"}
        assert rc.run_positions(big[0], knn) == can
    assert rc.run_positions(257, 129) >= {"full"} and rc.run_positions(257, 65) & {"full"} == set()
    assert max(rc.cuts(P, k) for P, k in rc.CHAIN_SHAPES) >= 3 and rc.cuts(257, 70) == 2 and rc.cuts(300, 64) == 0
    assert any(k == 0 for _, k in rc.CHAIN_SHAPES)
    # whole runs that END exactly on a wave's last lane (hi == 64) and partly dead last waves of whole runs
    assert rc.run_positions(65, 64) == {"whole", "dead_block"}
    assert "dead_wave" in rc.run_positions(65, 63)


def test_run_positions_by_hand():
    assert rc.run_positions(4, 16) == {"whole", "dead_block"}
    assert rc.run_positions(2, 48) == {"whole", "tail", "head", "dead_wave", "dead_block"}
    assert rc.run_positions(1, 130) == {"tail", "full", "head", "dead_wave", "dead_block"}
    assert rc.run_positions(3, 0) == set()


@pytest.fixture(scope="module")
def chain_oracles():
    out = {}
    for P, knn in rc.CHAIN_SHAPES:
        out[(P, knn, False)] = (rc.chain_case(P, knn),)
    for P, knn in rc.SENTINEL_SHAPES:
        out[(P, knn, True)] = (rc.chain_case(P, knn, hand_row=(P == 40)),)
    return {k: v + rc.chain_oracle(v[0]) for k, v in out.items()}


def test_ambiguity_cap_and_both_outcomes(chain_oracles):
    tiny_hit = tiny_miss = False
    for (P, knn, _), (case, cnt, mask, ambig) in chain_oracles.items():
        assert mask.shape == (P, knn) and cnt.shape == (P, 1)
        if P * knn >= 2000:
            assert ambig.mean() <= 1e-3, (P, knn)
            assert 0.02 < mask.mean() < 0.98, (P, knn, mask.mean())
        elif mask.size:
            tiny_hit |= bool(mask.any())
            tiny_miss |= bool((~mask).any())
    assert tiny_hit and tiny_miss


def test_sentinel_rows_hold_out_of_range_indices_and_the_oracle_skips_them(chain_oracles):
    seen = set()
    for (P, knn, sentinel), (case, cnt, mask, ambig) in chain_oracles.items():
        nbr = case["nbr"]
        bad = (nbr < 0) | (nbr >= P)
        if not sentinel:
            assert not bad.any()
            continue
        assert bad.any() and (nbr[bad] == -1).sum() == P * (knn - min(knn, P - 1))
        seen |= set(nbr[bad].tolist())
        assert not mask[bad].any() and not ambig[bad].any()
        assert np.array_equal(cnt[:, 0], mask.sum(1))
        # in-range pairs are those of the same rows without the bad slots
        keep = ~bad
        for g in range(P):
            cols = np.nonzero(keep[g])[0]
            if cols.size:
                sub = ro.sphere_ellipsoid_intersection(case["means3D"], case["scales"], case["rotations"],
                                                       np.tile(nbr[g, cols], (P, 1)), case["radius"], cols.size)
                assert np.array_equal(sub[1][g], mask[g, cols])
        # the second operator never scatters through them, whatever the mask byte says
        red1, idx1, msk1 = rc.with_self_column(cnt, nbr, mask)
        want = ro.min_redundancy(red1, idx1, msk1, knn + 1)
        forced = msk1.copy()
        forced[:, 1:][bad] = 1
        assert np.array_equal(ro.min_redundancy(red1, idx1, forced, knn + 1), want)
    assert seen >= {-1, -3, 40, 49}


def test_threshold_case_sits_exactly_on_v_equal_one():
    case, v = rc.threshold_case()
    assert v.shape == (9,) and (v[0::3] == 1).all() and (v[1::3] < 1).all() and (v[2::3] > 1).all()
    assert np.abs(v.astype(np.float64) - 1).max() <= 4 * np.finfo(F).eps        # the neighbours: a few ulp either side
    cnt, mask, ambig = rc.chain_oracle(case)
    assert mask[0].tolist() == [False, True, False] * 3 and cnt[0, 0] == 3       # v < 1 is strict
    assert ambig[0].all()                              # inside the band the general bar leaves out: compared exactly here
    assert np.array_equal(mask[1:, 0], np.array([False, True, False] * 3)) and (mask[1:] == mask[1:, :1]).all()


def test_min_redundancy_cases_hold_what_they_claim():
    cases = rc.min_redundancy_cases()
    red, nbr, msk = cases["repeated"]
    assert all(np.unique(r).size < r.size for r in nbr)
    red, nbr, msk = cases["all_false"]
    assert not msk.any() and (ro.min_redundancy(red, nbr, msk, nbr.shape[1]) == nbr.shape[0]).all()
    for name, (red, nbr, msk) in cases.items():
        P, k = nbr.shape
        out = ro.min_redundancy(red, nbr, msk, k)[:, 0]
        assert out.min() >= 0 and out.max() <= P
        if name.startswith("self_column"):
            assert np.unique(out).size > 5 and (out <= red).all()    # every entry at most its own value
        else:
            assert {0, rc.INT_MAX} <= set(red.tolist()), name
            if name != "all_false":
                assert (out == P).any() and (out < P).any(), name   # untouched / INT_MAX-only entries and real minima
    assert cases["self_column_65"][1].shape[1] == 65 and cases["self_column_129"][1].shape[1] == 129
    red, nbr, msk = cases["sentinel_masked"]
    bad = (nbr < 0) | (nbr >= nbr.shape[0])
    assert bad.any() and msk[bad].all()
    cleared = msk.copy()
    cleared[bad] = 0
    assert np.array_equal(ro.min_redundancy(red, nbr, msk, 9), ro.min_redundancy(red, nbr, cleared, 9))


# ---------------------------------------------------------------------------------------------------- pixel size
def test_pixel_cameras_take_both_branches_and_the_tie():
    w2ndc, inv, H, W = rc.pixel_cameras()
    assert W[0] > H[0] and W[1] < H[1] and W[2] == H[2]
    pts = rc.pixel_points(257)
    for c in range(3):
        got, ambig = ro.min_pixel_size(w2ndc[c:c + 1], inv[c:c + 1], pts, H[c:c + 1], W[c:c + 1], want_ambig=True)
        seen = (got[:, 0] != 10000) & ~ambig
        assert 20 < seen.sum() < 250                    # seen and unseen centres both occur
        # the other branch gives a different length: swapping H and W (for the square camera: one more column, what
        # `W >= H` would act on) changes every seen value by far more than 1e-5
        hw = (H[c:c + 1], W[c:c + 1] + 1) if c == 2 else (W[c:c + 1], H[c:c + 1])
        other = ro.min_pixel_size(w2ndc[c:c + 1], inv[c:c + 1], pts, *hw)
        assert (np.abs(other[seen, 0] / got[seen, 0] - 1) > 1e-2).all()


def test_border_table_has_on_and_outside_points_for_all_six_comparisons():
    w2ndc, inv, pts, H, W, rows = rc.border_case()
    assert pts.shape == (12, 3) and len(rows) == 12
    got = ro.min_pixel_size(w2ndc, inv, pts, H, W)[:, 0]
    have = set()
    for i, (axis, border, kind, value) in enumerate(rows):
        col = {"x": 0, "y": 1, "depth": 2}[axis]
        assert value == F(pts[i, col] * rc.PW)          # the kernel's one multiplication, in fp32
        away = 1 if border == 1 else -1
        if kind == "on":
            assert value == F(border) and got[i] != 10000
        else:
            assert value == np.nextafter(F(border), F(away) * F(np.inf)) and got[i] == 10000
        have.add((axis, border, kind))
    assert have == {(a, float(b), k) for a, _, b, _ in rc.BORDERS for k in ("on", "outside")} and len(have) == 12
    # the six borders are x, y at -1 and 1 and depth at 0 and 1
    assert {(a, float(b)) for a, _, b, _ in rc.BORDERS} == {("x", 1.0), ("x", -1.0), ("y", 1.0), ("y", -1.0),
                                                             ("depth", 1.0), ("depth", 0.0)}
    # the seen ones all get the same length: (2 / H) * pw  (W > H would be the x branch; 640 x 480 takes it)
    seen = got != 10000
    np.testing.assert_allclose(got[seen], F(2.0) / F(640) * rc.PW, rtol=1e-6)


def test_oracle_nonfinite_positions_are_unseen_and_nan_lengths_are_skipped():
    w2ndc, inv, H, W = rc.pixel_cameras()
    good, bad = rc.nonfinite_points()
    with np.errstate(all="ignore"):
        assert (ro.min_pixel_size(w2ndc, inv, good, H, W)[:, 0] != 10000).all()
        assert (ro.min_pixel_size(w2ndc, inv, bad, H, W) == 10000).all()
        # a camera whose inverse yields a NaN length leaves the minimum as it was, before or after a good camera
        nan_inv = np.full((1, 4, 4), np.nan, F)
        pts = rc.pixel_points(257)
        want = ro.min_pixel_size(w2ndc[:1], inv[:1], pts, H[:1], W[:1])
        for order in ((0, 1), (1, 0)):
            m = np.concatenate([w2ndc[:1], w2ndc[:1]])[list(order)]
            mi = np.concatenate([inv[:1], nan_inv])[list(order)]
            assert np.array_equal(ro.min_pixel_size(m, mi, pts, H[[0, 0]], W[[0, 0]]), want)
        assert (ro.min_pixel_size(w2ndc[:1], nan_inv, pts, H[:1], W[:1]) == 10000).all()


# ------------------------------------------------------------------------------------------------ pack_view_stats
@pytest.mark.parametrize("P", [255, 257])
def test_pack_cases_hold_every_kind(P):
    vg, radii = rc.pack_case(P)
    norm, vis, rad = rc.pack_want(vg, radii)
    assert set(radii.tolist()) == set(rc.PACK_RADII.tolist())
    assert np.isnan(vg[:, 2]).all()
    hidden = radii <= 0
    assert (np.isnan(vg[hidden, :2]).any(1)).any() and (np.isinf(vg[hidden, :2]).any(1)).any()
    assert not np.isnan(vg[~hidden, :2]).any()
    assert (norm[hidden].view(np.uint32) == 0).all() and not np.isnan(norm).any()
    v = ~hidden
    tiny = np.finfo(F).tiny
    assert ((np.abs(vg[v, 0]) < tiny) & (vg[v, 0] != 0)).any()               # denormal inputs
    assert ((norm[v] > 0) & (norm[v] < 1e-18)).any()                         # squares in the denormal range
    assert (np.signbit(vg[v, 0]) & (vg[v, 0] == 0)).any() and ((norm == 0) & v).any()
    assert (np.isinf(norm[v]) & np.isfinite(vg[v, :2]).all(1)).any()         # squares that overflow


# -------------------------------------------------------------------------------------------------- shard reduction
def _classify(u):
    """The rounding situations of f32_to_bf16_rne that the fp32 pattern u is in."""
    low, kept = u & 0xFFFF, (u >> 16) & 1
    out = set()
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return {"nan"}
    if low == 0x8000:
        out.add("tie_even" if kept == 0 else "tie_odd")
    if low == 0x7FFF:
        out.add("below_tie")
    if low == 0x8001:
        out.add("above_tie")
    if low >= 0x8000 and ((u >> 16) & 0x7F) == 0x7F and ((u >> 23) & 0xFF) < 0xFE:
        out.add("carry")
    if low >= 0x8000 and (u >> 16) & 0x7FFF == 0x7F7F:
        out.add("overflow")
    if u == 0x80000000:
        out.add("neg_zero")
    if (u & 0x7F800000) == 0 and (u & 0x007FFFFF):
        out.add("denormal")
    return out


SITUATIONS = {"tie_even", "tie_odd", "below_tie", "above_tie", "carry", "overflow", "neg_zero", "denormal", "nan"}


@pytest.mark.parametrize("world", rc.WORLDS)
def test_half_table_against_torch_and_in_both_halves(world):
    import torch
    words, layout = rc.half_table_words(world)
    halves = torch.from_numpy(words.view(np.int32).copy()).view(torch.bfloat16).view(world, -1).to(torch.float32)
    acc = halves[0].clone()
    for w in range(1, world):
        acc += halves[w]
    sums = acc.view(torch.int32).numpy().view(np.uint32).reshape(-1, 2)           # [word, (low, high)]
    conv = acc.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(-1, 2)
    found = {0: set(), 1: set()}
    for wd, names in enumerate(layout):
        for half, name in enumerate(names):
            if name is None:
                continue
            want = rc.HALF_TABLE[name][2]
            if want is None:
                assert (int(sums[wd, half]) & 0x7FFFFFFF) > 0x7F800000 and (conv[wd, half] & 0x7FFF) > 0x7F80, name
            else:
                assert conv[wd, half] == want, (name, hex(conv[wd, half]))
            found[half] |= _classify(int(sums[wd, half]))
    need = SITUATIONS if world >= 3 else SITUATIONS - {"below_tie", "above_tie"} if world == 2 else {"neg_zero", "denormal", "nan"}
    assert found[0] >= need and found[1] >= need, (need - found[0], need - found[1])
    if world == 1:
        # a signalling NaN goes in: the kernel's rule returns it quiet
        assert any(n == "nan_signalling_1rank" for n, _ in layout)


def test_every_half_table_entry_fits_some_world():
    assert set(rc.half_entries(3)) == set(rc.HALF_TABLE) == set(rc.half_entries(8))
    assert {len(v[0]) for v in rc.HALF_TABLE.values()} == {1, 2, 3}


@pytest.mark.parametrize("shard", rc.SHARDS)
def test_shard_borders_take_every_position(shard):
    b = rc.SHARD_BEGIN
    pos = rc.border_positions(shard)
    assert min(pos) < b and b in pos and b + shard in pos and max(pos) > b + shard       # before / first word / behind
    assert b + 1 in pos and b + shard - 1 in pos and b + shard // 2 in pos              # first, last word, middle
    pairs = rc.border_pairs(shard)
    assert all(h >= s for s, h in pairs) and any(h == s and b < s < b + shard or shard == 1 and h == s for s, h in pairs)
    counts = set()
    for s, h in pairs:
        n_sum = min(max(s - b, 0), shard)
        n_half = min(max(h - b, 0), shard) - n_sum
        counts.add((n_sum, n_half, shard - n_sum - n_half))
    assert (shard, 0, 0) in counts and (0, shard, 0) in counts and (0, 0, shard) in counts    # wholly in each region
    if shard > 2:
        assert any(a and c and d for a, c, d in counts)                                        # all three in one shard
    # the fill follows the regions, and the torch loop is bit-identical to a per-word numpy restatement of the maximum
    for world in (1, 3):
        s, h = b + shard // 2, b + shard
        recv = rc.shard_recv(world, shard, b, s, h)
        want, region = rc.shard_want(recv, b, s, h)
        assert (region == 0).sum() == shard // 2 and (region == 2).sum() == 0
        recv = rc.shard_recv(world, shard, b, 0, 0)
        want, region = rc.shard_want(recv, b, 0, 0)
        assert np.array_equal(want.view(np.int32), recv.view(np.int32).max(0)) and (region == 2).all()
        assert rc.shard_mismatches(want, want, region).size == 0


def test_int_and_float_specials_reach_the_named_values():
    ints = rc.int_words(3, 64).view(np.int32)
    assert (ints == rc.INT_MIN).any() and (ints == rc.INT_MAX).any() and (ints.max(0) < 0).any()
    # a column where the unsigned maximum differs from the signed one
    assert (ints.view(np.uint32).max(0).view(np.int32) != ints.max(0)).any()
    fl = rc.float_words(3, 64).view(F)
    with np.errstate(all="ignore"):
        s = (fl[0] + fl[1]) + fl[2]
    tiny = np.finfo(F).tiny
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
    assert ((np.abs(s) < tiny) & (s != 0)).any() and (np.signbit(s) & (s == 0)).any()
    assert (np.isinf(fl[0]) & np.isinf(fl[1]) & (fl[0] != fl[1])).any()                   # inf + -inf
