"""The six kernels of csrc/reduction_ops.hip at every edge of their index arithmetic and number formats: runs of
intersection_kernel in every position of a wave (whole, cut at the head, at the tail, covering a whole wave, partly dead
last wave and workgroup), knn == 0, reused (poisoned) outputs, the out-of-range neighbour rule of
include/r3dgs_reduction.h, both branches and the six frustum borders of min_pixel_size_kernel, non-finite positions,
pack_view_stats bit for bit, and the shard reductions over every region border, the signed maximum and each rounding
situation of the bfloat16 conversion.

The cases are tests/reduction_cases.py's; tests/test_reduction_edges_cpu.py proves without a GPU that they reach what
they claim.  Bars: those of tests/test_reduction_ops.py -- mask bit-exact off the oracle's ambiguous pairs (|v - 1| <
1e-5), counts equal to the kernel's own mask row sums everywhere and to the oracle's on rows without an ambiguous pair,
min_redundancy bit-exact against the oracle fed the device's own outputs, pixel sizes: same unseen set and rtol 1e-5 off
the ambiguity band (the identity-matrix border table: the set exactly, see reduction_cases.py); everything else bit for
bit.  Each test prints what it measured (`pytest -s`); profiles/reduction_edges_gpu_tests.txt records those lines."""
import numpy as np
import pytest

from oracle import reduction_ops as ro
from tests import reduction_cases as rc

pytestmark = pytest.mark.gpu

POISON_BYTE = 0x7F
POISON_WORD = 0x7F7F7F7F
GUARD = 16                                             # int32 words in front of, between and behind the carved outputs


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    from diff_gaussian_rasterization import _C
    return _C._lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class _Carved:
    """int32 slices inside ONE poisoned device buffer (every byte 0x7F), with GUARD poisoned words around each."""

    def __init__(self, *n_words):
        import torch
        self.spans, at = [], GUARD
        for n in n_words:
            self.spans.append((at, at + n))
            at += n + GUARD
        self.buf = torch.full((at,), POISON_WORD, dtype=torch.int32, device="cuda")

    def ptr(self, i):
        return self.buf.data_ptr() + 4 * self.spans[i][0]

    def read(self):
        """-> the slices as numpy int32 arrays, after checking that every word outside them is still poison."""
        host = self.buf.cpu().numpy()
        outside = np.ones(host.shape, bool)
        for a, b in self.spans:
            outside[a:b] = False
        touched = np.nonzero(outside & (host != POISON_WORD))[0]
        assert touched.size == 0, f"words {touched[:8]} outside the outputs {self.spans} were written"
        return [host[a:b].copy() for a, b in self.spans]


def _check(rc_code):
    assert rc_code >= 0, _lib().r3dgs_last_error().decode()


def _intersection(case):
    """r3dgs_sphere_ellipsoid_intersection into poisoned, caller-owned outputs -> (redundancy int32[P], mask uint8[P,knn])."""
    P, knn = case["nbr"].shape
    mask_words = (P * knn + 3) // 4
    out = _Carved(P, mask_words)
    dm, ds, dr = _dev(case["means3D"]), _dev(case["scales"]), _dev(case["rotations"])
    dn, drad = _dev(case["nbr"].reshape(-1)), _dev(case["radius"])
    _check(_lib().r3dgs_sphere_ellipsoid_intersection(P, knn, dm.data_ptr(), ds.data_ptr(), dr.data_ptr(),
                                                      dn.data_ptr() if knn else None, drad.data_ptr(), out.ptr(0),
                                                      out.ptr(1) if knn else None, _stream()))
    red, mask = out.read()
    mask = mask.view(np.uint8)
    assert (mask[P * knn:] == POISON_BYTE).all(), "bytes behind mask[P, knn] were written"
    mask = mask[:P * knn].reshape(P, knn)
    assert not (red == POISON_WORD).any(), f"redundancy entries {np.nonzero(red == POISON_WORD)[0][:8]} were never written"
    assert np.isin(mask, (0, 1)).all(), f"mask bytes other than 0 / 1: {np.unique(mask)[:8]} (0x7F = never written)"
    return red, mask


def _min_redundancy(red, nbr, mask):
    """r3dgs_min_redundancy into a poisoned slice with guarded words either side -> int32[P]."""
    P, k = nbr.shape
    out = _Carved(P)
    dr, dn, dk = _dev(red.reshape(-1).astype(np.int32)), _dev(nbr.reshape(-1)), _dev(mask.reshape(-1).astype(np.uint8))
    _check(_lib().r3dgs_min_redundancy(P, k, dr.data_ptr(), dn.data_ptr(), dk.data_ptr(), out.ptr(0), _stream()))
    (mn,) = out.read()                                   # checks the word in front of and the word behind min_redundancy
    assert not (mn == POISON_WORD).any(), "min_redundancy entries were never written"
    return mn


def _check_chain(label, case):
    P, knn = case["nbr"].shape
    cnt, mask, ambig = rc.chain_oracle(case)
    red, msk = _intersection(case)
    bad = (case["nbr"] < 0) | (case["nbr"] >= P)
    assert not msk[bad].any(), "a pair with an out-of-range neighbour index has its mask set"
    assert np.array_equal(msk.astype(bool)[~ambig], mask[~ambig])
    assert np.array_equal(red, msk.sum(1)), f"counts differ from the mask's row sums at {np.nonzero(red != msk.sum(1))[0][:8]}"
    clean = ~ambig.any(1)
    assert np.array_equal(red[clean], cnt[clean, 0])
    # the second operator on the first one's outputs plus the self column the caller prepends
    red1, idx1, msk1 = rc.with_self_column(red, case["nbr"], msk)
    mn = _min_redundancy(red1, idx1, msk1)
    assert np.array_equal(mn, ro.min_redundancy(red1, idx1, msk1, knn + 1)[:, 0])
    print(f"reduction_edges_gpu {label} P={P} knn={knn}: ambiguous pairs {int(ambig.sum())} of {ambig.size}, mask differs "
          f"from the oracle on {int((msk.astype(bool) != mask).sum())} (only ambiguous pairs may), "
          f"hit rate {msk.mean() if msk.size else 0:.3f}, run positions {sorted(rc.run_positions(P, knn))}")


@pytest.mark.parametrize("P,knn", rc.CHAIN_SHAPES)
def test_gpu_redundancy_chain_shapes(P, knn):
    _check_chain("chain", rc.chain_case(P, knn))


@pytest.mark.parametrize("P,knn", rc.SENTINEL_SHAPES)
def test_gpu_redundancy_chain_sentinel_rows(P, knn):
    """distIndex2's -1 in unfilled slots (P <= knn), and for P = 40 a hand-made row with -3, P and P + 9: no neighbour."""
    _check_chain("sentinel", rc.chain_case(P, knn, hand_row=(P == 40)))


def test_gpu_intersection_exactly_on_the_threshold():
    """v == 1 exactly is no hit, a distance one fp32 shorter is, one fp32 longer is not: identity rotations and power-of-two semi-axes make
    every operation exact, so the mask is held bit for bit inside the oracle's ambiguity band too."""
    case, v = rc.threshold_case()
    cnt, mask, ambig = rc.chain_oracle(case)
    red, msk = _intersection(case)
    assert np.array_equal(msk.astype(bool), mask), f"rows {np.nonzero((msk.astype(bool) != mask).any(1))[0]}; row 0: {msk[0]}"
    assert np.array_equal(red, cnt[:, 0]) and msk[0].tolist() == [0, 1, 0] * 3
    print(f"reduction_edges_gpu threshold table: v = {v[:3].tolist()} on each axis -> mask {msk[0, :3].tolist()}, exact")


@pytest.mark.parametrize("name", list(rc.min_redundancy_cases()))
def test_gpu_min_redundancy_alone(name):
    red, nbr, msk = rc.min_redundancy_cases()[name]
    mn = _min_redundancy(red, nbr, msk)
    want = ro.min_redundancy(red, nbr, msk, nbr.shape[1])[:, 0]
    assert np.array_equal(mn, want), f"entries {np.nonzero(mn != want)[0][:8]}: got {mn[mn != want][:8]}, want {want[mn != want][:8]}"
    print(f"reduction_edges_gpu min_redundancy {name} P={nbr.shape[0]} knn={nbr.shape[1]}: bit-exact, "
          f"{int((want == nbr.shape[0]).sum())} entries stay P, {int((want == 0).sum())} are 0")


# ---------------------------------------------------------------------------------------------------- pixel size
def _pixel_size(w2ndc, inv, pts, H, W):
    """r3dgs_min_pixel_size into a poisoned slice -> fp32[P]."""
    P, C = pts.shape[0], w2ndc.shape[0]
    out = _Carved(P)
    dm, di, dp, dh, dw = _dev(w2ndc.reshape(-1)), _dev(inv.reshape(-1)), _dev(pts), _dev(H), _dev(W)
    _check(_lib().r3dgs_min_pixel_size(P, C, dm.data_ptr() if C else None, di.data_ptr() if C else None, dp.data_ptr(),
                                       dh.data_ptr() if C else None, dw.data_ptr() if C else None, out.ptr(0), _stream()))
    (got,) = out.read()
    assert not (got == POISON_WORD).any(), "pixel_sizes entries were never written"
    return got.view(np.float32)


def _check_pixel(label, w2ndc, inv, pts, H, W):
    with np.errstate(all="ignore"):
        want, ambig = ro.min_pixel_size(w2ndc, inv, pts, H, W, want_ambig=True)
    got = _pixel_size(w2ndc, inv, pts, H, W)
    ok = ~ambig
    assert np.array_equal(got[ok] == 10000, want[ok, 0] == 10000)
    np.testing.assert_allclose(got[ok], want[ok, 0], rtol=1e-5)
    seen = ok & (want[:, 0] != 10000)
    rel = float(np.abs(got[seen] / want[seen, 0] - 1).max()) if seen.any() else 0.0
    print(f"reduction_edges_gpu pixel_size {label} P={pts.shape[0]} C={w2ndc.shape[0]}: {int(seen.sum())} seen, "
          f"{int(ambig.sum())} in the ambiguity band, worst relative deviation {rel:.3g} (bar 1e-5)")
    return got, want[:, 0]


@pytest.mark.parametrize("C", rc.PIXEL_C)
@pytest.mark.parametrize("P", rc.PIXEL_P)
def test_gpu_pixel_size_shapes(P, C):
    """Landscape, portrait and square cameras: both branches and the W == H tie; C == 1 takes each camera in turn."""
    for which in (range(3) if C == 1 else (0,)):
        got, want = _check_pixel(f"cameras {'LPS'[which] if C == 1 else 'LPS'[:C]}", *rc.pixel_case(P, C, which))
        if C == 0:
            assert (got == 10000).all()


def test_gpu_pixel_size_border_table():
    """Identity matrices: the computed value is one fp32 product, so the frustum decision is exact -- a point ON each of the
    six borders is seen (inclusive comparisons), the next fp32 OUTSIDE is not."""
    w2ndc, inv, pts, H, W, rows = rc.border_case()
    want = ro.min_pixel_size(w2ndc, inv, pts, H, W)[:, 0]
    got = _pixel_size(w2ndc, inv, pts, H, W)
    for i, (axis, border, kind, value) in enumerate(rows):
        assert (got[i] != 10000) == (kind == "on"), f"{axis} at {border}: the point whose value is {value!r} ({kind})"
    assert np.array_equal(got == 10000, want == 10000)
    np.testing.assert_allclose(got, want, rtol=1e-5)
    # the same table in a portrait and a square image: the other branch, same decisions
    for Wd, Hd in ((480, 640), (512, 512)):
        c = rc.border_case(Wd, Hd)
        g2 = _pixel_size(*c[:5])
        assert np.array_equal(g2 == 10000, want == 10000)
        np.testing.assert_allclose(g2, ro.min_pixel_size(*c[:5])[:, 0], rtol=1e-5)
    print(f"reduction_edges_gpu pixel_size border table: 6 on-border points seen, 6 one-ulp-outside points unseen, "
          f"worst relative deviation {float(np.abs(got[want != 10000] / want[want != 10000] - 1).max()):.3g}")


def test_gpu_pixel_size_nonfinite():
    """A NaN or infinite coordinate is unseen; a camera whose inverse yields a NaN length leaves the minimum as it was."""
    w2ndc, inv, H, W = rc.pixel_cameras()
    good, bad = rc.nonfinite_points()
    assert (_pixel_size(w2ndc, inv, good, H, W) != 10000).all()
    assert (_pixel_size(w2ndc, inv, bad, H, W) == 10000).all()
    for c in range(3):
        assert (_pixel_size(w2ndc[c:c + 1], inv[c:c + 1], bad, H[c:c + 1], W[c:c + 1]) == 10000).all()
    nan_inv = np.full((1, 4, 4), np.nan, np.float32)
    pts = rc.pixel_points(257)
    alone = _pixel_size(w2ndc[:1], inv[:1], pts, H[:1], W[:1])
    for order in ((0, 1), (1, 0)):
        m = np.concatenate([w2ndc[:1], w2ndc[:1]])[list(order)]
        mi = np.concatenate([inv[:1], nan_inv])[list(order)]
        both = _pixel_size(m, mi, pts, H[[0, 0]], W[[0, 0]])
        assert np.array_equal(both.view(np.int32), alone.view(np.int32))
    assert (_pixel_size(w2ndc[:1], nan_inv, pts, H[:1], W[:1]) == 10000).all()
    print("reduction_edges_gpu pixel_size non-finite: 9 NaN / inf positions unseen; a NaN-length camera changes no bit")


# ------------------------------------------------------------------------------------------------ pack_view_stats
@pytest.mark.parametrize("P", rc.PACK_P)
def test_gpu_pack_view_stats_bits(P):
    """Bit for bit against numpy fp32 sqrt(gx*gx + gy*gy) without contraction (the unit is built EXACT), `visible` and
    `radii_out` included; outputs poisoned, NaN in the column that is never read."""
    for seed in (range(12) if P == 1 else (0,)):
        vg, radii = rc.pack_case(P, seed)
        norm, vis, rad = rc.pack_want(vg, radii)
        out = _Carved(P, P, P)
        dv, dr = _dev(vg), _dev(radii)
        _check(_lib().r3dgs_pack_view_stats(P, dv.data_ptr(), dr.data_ptr(), out.ptr(0), out.ptr(1), out.ptr(2), _stream()))
        g_norm, g_vis, g_rad = out.read()
        assert np.array_equal(g_norm.view(np.uint32), norm.view(np.uint32)), (
            f"rows {np.nonzero(g_norm.view(np.uint32) != norm.view(np.uint32))[0][:8]}")
        assert np.array_equal(g_vis.view(np.uint32), vis.view(np.uint32)) and np.array_equal(g_rad, rad)
    print(f"reduction_edges_gpu pack_view_stats P={P}: grad_norm, visible, radii_out bit-exact (0 ulp)")


# -------------------------------------------------------------------------------------------------- shard reduction
def _reduce(recv, begin, sum_len, half_end=None):
    from diff_gaussian_rasterization import _C
    world, shard = recv.shape
    out = _Carved(shard)
    d = _dev(recv.view(np.int32).reshape(-1)).view(_torch_f32())
    o = out.buf[out.spans[0][0]:out.spans[0][1]].view(_torch_f32())
    if half_end is None:
        _C.reduce_shards(d, world, begin, sum_len, o)
    else:
        _C.reduce_shards_mixed(d, world, begin, sum_len, half_end, o)
    (got,) = out.read()
    return got.view(np.uint32)


def _torch_f32():
    import torch
    return torch.float32


@pytest.mark.parametrize("shard", rc.SHARDS)
@pytest.mark.parametrize("world", rc.WORLDS)
def test_gpu_reduce_shards_borders(world, shard):
    """fp32 SUM | int32 MAX with the border at every position of the shard: bit for bit against the rank-ordered loop."""
    b = rc.SHARD_BEGIN
    for rot, sum_len in enumerate(rc.border_positions(shard) * (6 if shard == 1 else 1)):
        recv = rc.shard_recv(world, shard, b, sum_len, sum_len, rot=rot, seed=rot)
        want, region = rc.shard_want(recv, b, sum_len, sum_len)
        got = _reduce(recv, b, sum_len)
        bad = rc.shard_mismatches(got, want, region)
        assert bad.size == 0, (f"sum_len={sum_len}: words {bad[:6]} (regions {region[bad[:6]]}): got "
                               f"{[hex(x) for x in got[bad[:6]]]}, want {[hex(x) for x in want[bad[:6]]]}")
    print(f"reduction_edges_gpu reduce_shards world={world} shard={shard}: bit-exact at {len(rc.border_positions(shard))} borders")


@pytest.mark.parametrize("shard", rc.SHARDS)
@pytest.mark.parametrize("world", rc.WORLDS)
def test_gpu_reduce_shards_mixed_borders(world, shard):
    """fp32 SUM | bfloat16 pairs | int32 MAX with both borders at every position independently, half_end == sum_len
    included (then it must be r3dgs_reduce_shards, bit for bit)."""
    b = rc.SHARD_BEGIN
    for rot, (sum_len, half_end) in enumerate(rc.border_pairs(shard)):
        recv = rc.shard_recv(world, shard, b, sum_len, half_end, rot=rot, seed=rot)
        want, region = rc.shard_want(recv, b, sum_len, half_end)
        got = _reduce(recv, b, sum_len, half_end)
        bad = rc.shard_mismatches(got, want, region)
        assert bad.size == 0, (f"sum_len={sum_len} half_end={half_end}: words {bad[:6]} (regions {region[bad[:6]]}): got "
                               f"{[hex(x) for x in got[bad[:6]]]}, want {[hex(x) for x in want[bad[:6]]]}")
        if half_end == sum_len:
            assert np.array_equal(got, _reduce(recv, b, sum_len))
    print(f"reduction_edges_gpu reduce_shards_mixed world={world} shard={shard}: bit-exact at {len(rc.border_pairs(shard))} "
          f"border pairs")


@pytest.mark.parametrize("world", rc.WORLDS)
def test_gpu_reduce_shards_mixed_half_table(world):
    """Every rounding situation of the bfloat16 conversion (ties to even and to odd, one fp32 ulp either side, the carry
    into the exponent, overflow to inf, -0.0, denormals, NaN) in the low and in the high half of a word, the whole shard
    in the half region; the expected patterns are the table's own (checked against torch on the CPU)."""
    words, layout = rc.half_table_words(world)
    shard = words.shape[1]
    assert shard <= 257
    b = rc.SHARD_BEGIN
    got = _reduce(words, b, 0, b + shard + 7)
    want, region = rc.shard_want(words, b, 0, b + shard + 7)
    assert (region == 1).all()
    for wd, names in enumerate(layout):
        for half, name in enumerate(names):
            if name is None:
                continue
            h = int(got[wd] >> np.uint32(16 * half)) & 0xFFFF
            exp = rc.HALF_TABLE[name][2]
            if exp is None:
                assert (h & 0x7FC0) == 0x7FC0, f"{name} ({('low', 'high')[half]} half): {h:#06x} is no quiet NaN"
            else:
                assert h == exp, f"{name} ({('low', 'high')[half]} half): got {h:#06x}, want {exp:#06x}"
    assert rc.shard_mismatches(got, want, region).size == 0
    print(f"reduction_edges_gpu reduce_shards_mixed half table world={world}: {len(rc.half_entries(world))} entries x 2 halves "
          f"bit-exact")
