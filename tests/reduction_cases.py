"""TEST INFRASTRUCTURE ONLY -- the cases that tests/test_reduction_edges_gpu.py (the six kernels of
csrc/reduction_ops.hip) and tests/test_reduction_edges_cpu.py (the coverage claims, on the index arithmetic and the
oracle alone) share.

Redundancy chain.  intersection_kernel has one lane per (Gaussian, neighbour) pair, 64 lanes per wave, 256 per
workgroup; the pairs of Gaussian g are the run [g * knn, (g + 1) * knn).  The part of a run inside one wave is one of
  whole   the run starts and ends in this wave (plain store of the count);
  tail    the run starts here and goes on in the next wave        (seg_lo >= 0, seg_hi > 64: atomic);
  head    the run started in an earlier wave and ends here        (seg_lo <  0, seg_hi <= 64: atomic);
  full    the run covers the wave and more on both sides          (seg_lo <  0, seg_hi > 64: atomic, needs knn >= 66);
and the last wave / workgroup of the launch is partly dead when P * knn is no multiple of 64 / 256.  `run_positions`
derives these from P and knn alone.

Pixel size.  BORDER_* is a table for w2ndc = w2ndc_inv = identity: then hom = (x, y, z, 1) exactly, pw = 1 / (1 + 1e-7f)
in fp32, and n = coordinate * pw is ONE fp32 multiplication: every other product is by 0 or 1, so no contraction can
change a bit and the frustum decision is compared exactly, the oracle's ambiguity band included.

bfloat16 table.  HALF_TABLE lists per-rank bfloat16 bit patterns whose fp32 sum in rank order lands on each rounding
situation of f32_to_bf16_rne; `half_table_words` packs every entry once into the low and once into the high half."""
import numpy as np

import synth_scene as ss
from oracle import reduction_ops as ro

F = np.float32
WAVE, BLOCK = 64, 256
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# ---------------------------------------------------------------------------------------------- redundancy chain
KNNS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200)
SMALL_P = (1, 2, 3, 64, 65, 257)
LARGE_P = {127: 1000, 128: 777, 129: 500, 200: 333}   # one larger P per knn >= 127 (odd pair totals, many offsets)
CHAIN_SHAPES = [(P, k) for k in KNNS for P in SMALL_P if P > k] + [(P, k) for k, P in LARGE_P.items()]
SENTINEL_SHAPES = [(P, k) for P in (1, 2, 5, 40) for k in (8, 64)]
POSITIONS = ("whole", "tail", "head", "full", "dead_wave", "dead_block")


def run_positions(P, knn):
    """Which positions the runs of a (P, knn) launch take, from the index arithmetic of intersection_kernel alone."""
    found = set()
    total = P * knn
    if knn == 0:
        return found
    if total % WAVE:
        found.add("dead_wave")
    if total % BLOCK:
        found.add("dead_block")
    for g in range(P):
        a, b = g * knn, (g + 1) * knn                  # the run, [a, b)
        for wave in range(a // WAVE, (b - 1) // WAVE + 1):
            seg_lo, seg_hi = a - wave * WAVE, b - wave * WAVE
            if seg_lo >= 0 and seg_hi <= WAVE:
                found.add("whole")
            elif seg_lo >= 0:
                found.add("tail")
            elif seg_hi <= WAVE:
                found.add("head")
            else:
                found.add("full")
    return found


def cuts(P, knn):
    """The largest number of wave boundaries inside one run."""
    return max(((g + 1) * knn - 1) // WAVE - g * knn // WAVE for g in range(P)) if knn else 0


def _scene(P, seed):
    cam = ss.make_camera(400, 300, 350.0)
    return ss.make_gaussians(P, cam, seed=seed, behind_frac=0.05)


def chain_case(P, knn, hand_row=False):
    """-> dict(means3D, scales, rotations, nbr int32[P,knn], radius fp32[P,1]).  Neighbours by ro.knn_bruteforce (-1 in
    the slots that P - 1 < knn leaves unfilled); radius = the median FILLED neighbour distance times a log-normal factor,
    as tests/test_reduction_ops.py chooses it, so that both outcomes occur.  hand_row: row 1 additionally gets -3, P and
    P + 9 among its valid indices."""
    g = _scene(P, seed=1000 * P + knn)
    rng = np.random.default_rng(1000 * P + knn)
    filled = min(knn, P - 1)
    if knn:
        d2, nbr = ro.knn_bruteforce(g["means3D"], knn)
    else:
        d2, nbr = np.zeros((P, 0), F), np.zeros((P, 0), np.int32)
    base = np.sqrt(d2[:, filled // 2:filled // 2 + 1]) if filled else np.ones((P, 1), F)
    radius = (base * np.exp(rng.normal(0, 0.5, (P, 1)))).astype(F)
    nbr = np.ascontiguousarray(nbr, np.int32)
    if hand_row:
        nbr[1, [0, 3, 5]] = [-3, P, P + 9]
    return dict(means3D=g["means3D"], scales=g["scales"], rotations=g["rotations"], nbr=nbr, radius=radius)


def threshold_case():
    """The `v < 1` decision exactly ON its threshold.  Identity rotations, every scale 1.5 and every radius 0.5 (so the
    augmented semi-axes are exactly 2 and 1 / (a * a) is exactly 0.25), Gaussian 0 at the origin and nine others on the
    x, y and z axes at distance 2 (v == 1 exactly: NO hit), the next fp32 below 2 (hit) and the next above (no hit).
    Every product is by 0, 1 or a power of two except the one square, so no contraction can change a bit and the mask
    is compared exactly although the oracle calls these pairs ambiguous.  Row 0 lists the nine, the others list
    Gaussian 0 nine times (the same distances seen from the other end).
    -> (case dict, v fp32[9] of row 0 as computed here)"""
    two = F(2.0)
    dist = [two, np.nextafter(two, F(0)), np.nextafter(two, F(3))]
    means = np.zeros((10, 3), F)
    for axis in range(3):
        for k, d in enumerate(dist):
            means[1 + 3 * axis + k, axis] = d
    nbr = np.zeros((10, 9), np.int32)
    nbr[0] = np.arange(1, 10)
    rot = np.tile(np.array([[1, 0, 0, 0]], F), (10, 1))
    case = dict(means3D=means, scales=np.full((10, 3), 1.5, F), rotations=rot, nbr=nbr, radius=np.full((10, 1), 0.5, F))
    d = np.array(dist * 3, F)
    v = ((d * d).astype(F) * (F(1.0) / F(F(2.0) * F(2.0)))).astype(F)
    return case, v


def chain_oracle(c):
    P, knn = c["nbr"].shape
    return ro.sphere_ellipsoid_intersection(c["means3D"], c["scales"], c["rotations"], c["nbr"], c["radius"], knn)


def with_self_column(red, nbr, mask):
    """What scene/__init__.py:143-174 hands the second operator: count + 1, the Gaussian itself as column 0, mask 1."""
    P = nbr.shape[0]
    idx1 = np.concatenate([np.arange(P, dtype=np.int32).reshape(P, 1), nbr.astype(np.int32)], 1)
    msk1 = np.concatenate([np.ones((P, 1), np.uint8), mask.astype(np.uint8)], 1)
    return (red.reshape(P, 1) + 1).astype(np.int32), np.ascontiguousarray(idx1), np.ascontiguousarray(msk1)


def min_redundancy_cases():
    """name -> (redundancy int32[P], nbr int32[P,k], mask uint8[P,k]) for r3dgs_min_redundancy on its own."""
    out = {}
    rng = np.random.default_rng(77)
    specials = np.array([0, INT_MAX, 1, 5, INT_MAX, 0, 17], np.int32)

    def red(P):
        return specials[rng.integers(0, specials.size, P)]

    P, k = 257, 7                                      # few distinct targets, repeated inside a row
    nbr = rng.integers(0, 9, (P, k)).astype(np.int32)
    nbr[:, 3] = nbr[:, 1]
    out["repeated"] = (red(P), nbr, (rng.random((P, k)) < 0.6).astype(np.uint8))
    P, k = 64, 4
    out["all_false"] = (red(P), rng.integers(0, P, (P, k)).astype(np.int32), np.zeros((P, k), np.uint8))
    for k in (65, 129):                                # knn + 1: the self column pushes every run across a wave
        P = 300 if k == 65 else 130
        nbr = rng.integers(0, P, (P, k)).astype(np.int32)
        nbr[:, 0] = np.arange(P)
        msk = (rng.random((P, k)) < 0.3).astype(np.uint8)
        msk[:, 0] = 1
        out[f"self_column_{k}"] = (rng.integers(1, k + 1, P).astype(np.int32), nbr, msk)   # count + 1, as chained
    P, k = 257, 3                                      # only the extreme values: the result is 0, or P (= min(P, INT_MAX))
    out["extremes"] = (np.where(rng.random(P) < 0.5, 0, INT_MAX).astype(np.int32),
                       rng.integers(0, P, (P, k)).astype(np.int32), (rng.random((P, k)) < 0.5).astype(np.uint8))
    P, k = 40, 9                                       # out-of-range indices WITH the mask byte set
    nbr = rng.integers(0, P, (P, k)).astype(np.int32)
    msk = (rng.random((P, k)) < 0.5).astype(np.uint8)
    bad = rng.random((P, k)) < 0.3
    nbr[bad] = rng.choice(np.array([-1, -3, P, P + 9, INT_MIN, INT_MAX], np.int32), int(bad.sum()))
    msk[bad] = 1
    out["sentinel_masked"] = (red(P), nbr, msk)
    return out


# ---------------------------------------------------------------------------------------------------- pixel size
PIXEL_P = (1, 255, 256, 257)
PIXEL_C = (0, 1, 3)


def pixel_cameras():
    """Landscape (W > H), portrait (W < H) and square with non-square pixels (W == H: the tie takes the `else` branch,
    and fx != fy makes the two branches differ by far more than the bar)."""
    rng = np.random.default_rng(5)
    cams = [ss.make_camera(400, 300, 350.0, seed=1), ss.make_camera(300, 400, 350.0, seed=2),
            ss.Camera(256, 256, 300.0, 220.0, ss.rot_xyz(*rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.3, 0.3, 3))]
    w2ndc = np.stack([c.full_proj_transform for c in cams]).astype(F)
    inv = np.stack([np.linalg.inv(c.full_proj_transform.astype(np.float64)) for c in cams]).astype(F)
    H = np.array([c.image_height for c in cams], np.int32)
    W = np.array([c.image_width for c in cams], np.int32)
    return w2ndc, inv, H, W


def pixel_points(P):
    cam = ss.make_camera(400, 300, 350.0)
    return ss.make_gaussians(P, cam, seed=31 * P, behind_frac=0.1)["means3D"]


def pixel_case(P, C, which=0):
    """C cameras of the three (C == 1: the one numbered `which`)."""
    w2ndc, inv, H, W = pixel_cameras()
    sel = [which % 3] if C == 1 else list(range(C))
    return w2ndc[sel], inv[sel], pixel_points(P), H[sel], W[sel]


PW = F(1.0) / (F(1.0) + F(0.0000001))                 # 1 / (hom.w + 1e-7) for hom.w == 1, in fp32
BORDER_INTERIOR = (F(0.25), F(-0.5), F(0.5))
# (axis, border, direction that leaves the frustum): the six comparisons of min_pixel_size_kernel
BORDERS = (("x", 0, F(1), +1), ("x", 0, F(-1), -1), ("y", 1, F(1), +1), ("y", 1, F(-1), -1),
           ("depth", 2, F(1), +1), ("depth", 2, F(0), -1))


def ndc(coord):
    """What the kernel computes from one coordinate under the identity matrix: a single fp32 product."""
    return F(F(coord) * PW)


def _search(border, want):
    """The fp32 coordinate nearest `border` whose ndc() is exactly `want`, searched over the neighbouring floats."""
    x = F(border)
    cands = [x]
    up = down = x
    for _ in range(16):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        cands += [up, down]
    for c in cands:
        if ndc(c) == want:
            return c
    raise AssertionError(f"no fp32 coordinate near {border} maps onto {want}")


def border_table():
    """-> (points fp32[12,3], rows): for each of the six comparisons a point whose computed value is exactly ON the border
    (inside: the comparisons are inclusive) and one whose value is the next fp32 OUTSIDE it; the other two coordinates sit
    well inside.  rows[i] = (axis, border, 'on' | 'outside', the computed value)."""
    pts, rows = [], []
    for axis, col, border, away in BORDERS:
        outside = np.nextafter(border, F(away) * F(np.inf))
        for kind, want in (("on", border), ("outside", outside)):
            p = list(BORDER_INTERIOR)
            p[col] = _search(border, want)
            pts.append(p)
            rows.append((axis, float(border), kind, ndc(p[col])))
    return np.array(pts, F), rows


def border_case(W=640, H=480):
    eye = np.eye(4, dtype=F).reshape(1, 4, 4)
    pts, rows = border_table()
    return eye, eye.copy(), pts, np.array([H], np.int32), np.array([W], np.int32), rows


def nonfinite_points():
    """Points a camera of pixel_cameras() sees, each with one coordinate replaced by NaN, +inf or -inf."""
    w2ndc, inv, H, W = pixel_cameras()
    pts = pixel_points(257)
    seen = ro.min_pixel_size(w2ndc[:1], inv[:1], pts, H[:1], W[:1])[:, 0] != 10000
    good = pts[seen][:9].copy()
    assert good.shape[0] == 9
    bad = good.copy()
    for i, v in enumerate([np.nan, np.inf, -np.inf] * 3):
        bad[i, i // 3] = v
    return good, bad


# ------------------------------------------------------------------------------------------------ pack_view_stats
PACK_P = (1, 255, 256, 257)
PACK_RADII = np.array([-5, 0, 1, INT_MAX], np.int32)


def pack_case(P, seed=0):
    """-> (viewspace_grad fp32[P,3], radii int32[P]).  Row kinds in turn: normal, denormal inputs, results in the denormal
    range, +-0, squares that overflow, infinities in visible rows; rows with radii <= 0 additionally get NaN / inf in a
    third of the cases; column 2 is NaN throughout (never read)."""
    rng = np.random.default_rng(100 * P + seed)
    vg = rng.normal(0, 1, (P, 3)).astype(F)
    kind = (np.arange(P) + seed) % 6
    tiny = F(1e-40) * rng.integers(-9, 10, (P, 2)).astype(F)
    vg[kind == 1, :2] = tiny[kind == 1]
    vg[kind == 2, :2] = (rng.normal(0, 1, (P, 2)) * 10.0 ** rng.uniform(-23, -19, (P, 2))).astype(F)[kind == 2]
    vg[kind == 3, :2] = rng.choice(np.array([0.0, -0.0], F), (P, 2))[kind == 3]
    vg[kind == 4, :2] = (rng.normal(0, 1, (P, 2)) * 10.0 ** rng.uniform(18, 38, (P, 2))).astype(F)[kind == 4]
    vg[kind == 5, 0] = rng.choice(np.array([np.inf, -np.inf, 3.0], F), P)[kind == 5]
    radii = PACK_RADII[rng.integers(0, 4, P)]
    if P > 1:
        radii[:4] = PACK_RADII[:min(P, 4)]
    hidden = np.nonzero(radii <= 0)[0]
    for j, i in enumerate(hidden):
        if j % 3 == 0:
            vg[i, :2] = [[np.nan, 1.0], [np.inf, np.nan], [-np.inf, np.inf], [2.0, np.nan]][(j // 3) % 4]
    vg[:, 2] = np.nan
    return vg, np.ascontiguousarray(radii)


def pack_want(vg, radii):
    """numpy fp32, every operation rounded on its own (no contraction), correctly rounded sqrt."""
    gx, gy = vg[:, 0].astype(F), vg[:, 1].astype(F)
    with np.errstate(all="ignore"):
        xx, yy = (gx * gx).astype(F), (gy * gy).astype(F)
        norm = np.sqrt((xx + yy).astype(F)).astype(F)
    vis = radii > 0
    return np.where(vis, norm, F(0.0)).astype(F), vis.astype(F), radii.copy()


# -------------------------------------------------------------------------------------------------- shard reduction
WORLDS = (1, 2, 3, 8)
SHARDS = (1, 255, 256, 257)
SHARD_BEGIN = 1000


def border_positions(shard, begin=SHARD_BEGIN):
    """A region border before the shard, exactly on its first word (two ways: the first word is the first of the next
    region / the last of this one), in its middle, exactly on its last word (two ways) and behind it."""
    pos = [0, begin - 3, begin, begin + 1, begin + shard // 2, begin + shard - 1, begin + shard, begin + shard + 5]
    return sorted(set(pos))


def border_pairs(shard, begin=SHARD_BEGIN):
    """(sum_len, half_end) with each border at every position independently (half_end >= sum_len is the ABI's rule)."""
    pos = border_positions(shard, begin)
    return [(s, h) for s in pos for h in pos if h >= s]


def _bits(x):
    return np.array(x, F).view(np.uint32)


FLOAT_SPECIALS = [       # per-rank values (cycled over the ranks) of one fp32 SUM column
    [0.0, -0.0], [-0.0], [1e-45, 1e-45, -1e-45], [1e-39, 2e-39], [np.inf, 1.0, 2.0], [np.inf, -np.inf, 1.0],
    [-np.inf, -np.inf], [np.nan, 1.0, 2.0], [3e38, 3e38], [1.0, 1e-8, -1.0], [1.17549435e-38, -1.1754942e-38],
]
INT_SPECIALS = [         # per-rank words of one int32 MAX column
    [-5, -7, -6], [INT_MIN, INT_MIN + 1], [INT_MIN], [INT_MAX, -1, 0], [-1, 0], [-1, -2 ** 30], [0, INT_MIN, 7],
    [INT_MIN, INT_MAX], [-2 ** 31 + 5, -3, -2 ** 20],
]


def _column(spec, world):
    return [spec[w % len(spec)] for w in range(world)]


def float_words(world, n, rot=0, seed=0):
    """uint32[world, n] fp32 bit patterns: special columns and random ones alternate, starting at special `rot`."""
    rng = np.random.default_rng(seed + 1)
    out = (rng.normal(0, 1, (world, n)) * 10.0 ** rng.uniform(-3, 3, (1, n))).astype(F)
    for j in range(n):
        s = j + rot
        if s % 2 == 0:
            out[:, j] = np.array(_column(FLOAT_SPECIALS[(s // 2) % len(FLOAT_SPECIALS)], world), F)
    return out.view(np.uint32)


def int_words(world, n, rot=0, seed=0):
    """uint32[world, n] int32 bit patterns over the whole signed range, special columns in between."""
    rng = np.random.default_rng(seed + 2)
    out = rng.integers(INT_MIN, INT_MAX, (world, n), dtype=np.int64, endpoint=True)
    neg = rng.random(n) < 0.3                          # columns of negative words only: an unsigned max orders them wrongly
    out[:, neg] = -np.abs(out[:, neg]) - 1
    out = np.clip(out, INT_MIN, INT_MAX)
    for j in range(n):
        s = j + rot
        if s % 2 == 0:
            out[:, j] = _column(INT_SPECIALS[(s // 2) % len(INT_SPECIALS)], world)
    return out.astype(np.int32).view(np.uint32)


# name -> (per-rank bfloat16 bit patterns in rank order, pad pattern for the remaining ranks, the result's bit pattern or
# None for "a quiet NaN").  The fp32 sum of the widened values in rank order lands where the name says.
HALF_TABLE = {
    "tie_even":        ([0x3F80, 0x3B80], 0x0000, 0x3F80),          # 1 + 2^-8 = 0x3F808000: kept bit even, down
    "tie_odd":         ([0x3F81, 0x3B80], 0x0000, 0x3F82),          # 0x3F818000: kept bit odd, up
    "below_tie":       ([0x3F80, 0x3B80, 0xB400], 0x0000, 0x3F80),  # 0x3F807FFF
    "above_tie":       ([0x3F80, 0x3B80, 0x3400], 0x0000, 0x3F81),  # 0x3F808001
    "below_tie_odd":   ([0x3F81, 0x3B80, 0xB400], 0x0000, 0x3F81),  # 0x3F817FFF
    "above_tie_odd":   ([0x3F81, 0x3B80, 0x3400], 0x0000, 0x3F82),  # 0x3F818001
    "carry":           ([0x3FFF, 0x3B80], 0x0000, 0x4000),          # 0x3FFF8000: mantissa 0x7F carries into the exponent
    "overflow":        ([0x7F7F, 0x7B00], 0x0000, 0x7F80),          # largest finite + half its ulp: 0x7F7F8000 -> inf
    "neg_overflow":    ([0xFF7F, 0xFB00], 0x0000, 0xFF80),
    "neg_zero":        ([0x8000, 0x8000], 0x8000, 0x8000),
    "neg_zero_1rank":  ([0x8000], 0x8000, 0x8000),
    "denormal":        ([0x0081, 0x8080], 0x0000, 0x0001),          # 2^-126 (1 + 2^-7) - 2^-126 = 2^-133
    "denormal_sum":    ([0x0001, 0x0001], 0x0000, 0x0002),
    "denormal_1rank":  ([0x0043], 0x0000, 0x0043),
    "nan_inf_minus_inf": ([0x7F80, 0xFF80], 0x0000, None),
    "nan_quiet":       ([0x7FC0, 0x3F80], 0x0000, None),
    "nan_quiet_1rank": ([0x7FC5], 0x0000, None),
    "nan_signalling_1rank": ([0x7F81], 0x0000, None),               # must come back quiet
    "nan_negative_1rank": ([0xFFFF], 0x0000, None),
    "inf_1rank":       ([0x7F80], 0x0000, 0x7F80),
    "plain":           ([0x3FC0, 0x4010, 0xBF00], 0x0000, 0x4050),          # 1.5 + 2.25 - 0.5 = 3.25, exact
}
HALF_FILL = 0x3FC0                                     # 1.5 in every rank: the other half of a table word


def half_entries(world):
    """The table entries that `world` ranks can hold."""
    return [k for k, (vals, _, _) in HALF_TABLE.items() if len(vals) <= world]


def half_column(name, world):
    vals, pad, _ = HALF_TABLE[name]
    return np.array(list(vals) + [pad] * (world - len(vals)), np.uint32)


def half_table_words(world):
    """-> (uint32[world, 2 * n] words, layout): entry i in the LOW half of word 2i (high half = 1.5 per rank) and in the
    HIGH half of word 2i + 1; layout[word] = (name in the low half or None, name in the high half or None)."""
    names = half_entries(world)
    words = np.zeros((world, 2 * len(names)), np.uint32)
    layout = []
    for i, name in enumerate(names):
        col = half_column(name, world)
        words[:, 2 * i] = col | (np.uint32(HALF_FILL) << np.uint32(16))
        words[:, 2 * i + 1] = np.uint32(HALF_FILL) | (col << np.uint32(16))
        layout += [(name, None), (None, name)]
    return words, layout


def half_words(world, n, rot=0, seed=0):
    """uint32[world, n] bfloat16 pairs: the table's words (cyclically from word `rot`) and random pairs alternate."""
    rng = np.random.default_rng(seed + 3)
    rnd = (rng.normal(0, 3, (world, n, 2)).astype(F).view(np.uint32) >> np.uint32(16)).astype(np.uint32)
    out = rnd[..., 0] | (rnd[..., 1] << np.uint32(16))
    table, _ = half_table_words(world)
    for j in range(n):
        s = j + rot
        if s % 2 == 0:
            out[:, j] = table[:, (s // 2) % table.shape[1]]
    return out


def shard_recv(world, shard, begin, sum_len, half_end, rot=0, seed=0):
    """uint32[world, shard]: every word filled according to the region its buffer index begin + j lies in."""
    e = begin + np.arange(shard)
    out = int_words(world, shard, rot, seed)
    fl, hf = float_words(world, shard, rot, seed), half_words(world, shard, rot, seed)
    out[:, e < half_end] = hf[:, e < half_end]
    out[:, e < sum_len] = fl[:, e < sum_len]
    return np.ascontiguousarray(out)


def shard_want(recv, begin, sum_len, half_end):
    """The rank-ordered torch loop of tests/test_reduction_ops.py -> (uint32[shard] words, region int[shard]: 0 sum,
    1 half, 2 max)."""
    import torch
    world, shard = recv.shape
    e = begin + np.arange(shard)
    region = np.where(e < sum_len, 0, np.where(e < half_end, 1, 2))
    t = torch.from_numpy(recv.view(np.int32).copy())
    f = t.view(torch.float32)
    acc = f[0].clone()
    for w in range(1, world):
        acc += f[w]
    h = t.view(torch.bfloat16).view(world, 2 * shard).to(torch.float32)
    hacc = h[0].clone()
    for w in range(1, world):
        hacc += h[w]
    half = hacc.to(torch.bfloat16).view(torch.int32)
    mx = t.amax(0)
    want = np.where(region == 0, acc.view(torch.int32).numpy(), np.where(region == 1, half.numpy(), mx.numpy()))
    return want.astype(np.int32).view(np.uint32), region


def _is_nan32(u):
    return (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def _is_nan16(h):
    return (h & np.uint32(0x7FFF)) > np.uint32(0x7F80)


def shard_mismatches(got, want, region):
    """Indices where `got` (uint32 words) is not `want` bit for bit.  A NaN has no defined payload: where the loop gives
    a NaN, an fp32 word must be a NaN and a bfloat16 half must be a QUIET NaN (f32_to_bf16_rne's rule)."""
    got, want = got.astype(np.uint32), want.astype(np.uint32)
    ok = got == want
    f = region == 0
    ok |= f & _is_nan32(want) & _is_nan32(got)
    halves_ok = np.ones(got.shape, bool)
    for shift in (np.uint32(0), np.uint32(16)):
        g, w = (got >> shift) & np.uint32(0xFFFF), (want >> shift) & np.uint32(0xFFFF)
        halves_ok &= (g == w) | (_is_nan16(w) & ((g & np.uint32(0x7FC0)) == np.uint32(0x7FC0)))
    ok |= (region == 1) & halves_ok
    return np.nonzero(~ok)[0]
