"""TEST INFRASTRUCTURE ONLY -- the cases, the one-update oracle and the derived bar that tests/test_kmeans_gpu.py
(the HIP operator) and tests/test_kmeans_cpu.py (the cases' preconditions and the bar itself) share.

One update at a time: trajectories of k updates are not comparable (one ulp in a centre can move a value that sits on
a midpoint, and two correct runs then diverge), so update k of the library is held to ONE oracle update applied to
the library's own centres after k - 1 updates.

The oracle update (oracle/reduction_ops.py: kmeans, one turn of its loop): a = kmeans_assign(v, c_prev); float64 sums
by np.bincount, rounded to fp32, divided by the fp32 size; NaN -> 0.

The bar, per centre with a finite `want`:  |got - want| <= 2 ulp32(want) + 2^-50 * sum|v| / size_i
  * 2 ulp32(want): one fp32 rounding of the sum and one of the quotient;
  * 2^-50 * sum|v| / size_i: the library forms a cluster's sum as the difference of two entries of an fp64 prefix sum
    of the sorted values; each entry of a parallel (blocked) scan carries a few 2^-53 relative roundings of at most
    sum|v| (the finite values: the infinite ones stay out of the prefix), and the difference is divided by the size.
Derived, not measured.  Where `want` is infinite, where the cluster is empty, and where the oracle's quotient is NaN
(a cluster holding both infinities -> 0), `got` must be equal."""
import numpy as np

from oracle import reduction_ops as ro

F = np.float32
FLT_MAX = np.finfo(F).max

# every n and every centre count of the segment pass's edges (8 values per thread, 2048 per workgroup, the float4 path
# against the tail path, the closing add) and of the centre sort's power-of-two padding; n = 0 has a test of its own
SHAPES = [(1, 1), (1, 2), (1, 64), (7, 1), (7, 63), (7, 1024), (8, 2), (8, 65), (9, 64), (9, 257), (2047, 63),
          (2047, 256), (2048, 1), (2048, 64), (2048, 1024), (2049, 2), (2049, 65), (2049, 257), (4097, 63),
          (4097, 256), (4097, 1024), (65537, 1), (65537, 65), (65537, 256), (65537, 257), (65537, 1024)]
SET_SIZES = (4097, 65537)
SET_CENTRES = 256


def ulp32(x):
    """Spacing of fp32 at |x| (float64 array), 2^-149 in the subnormal range."""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.where(m == 0, -149, np.maximum(e - 24, -149)))


def oracle_update(v, c_prev, a=None):
    """-> (want fp32[nc], sizes int[nc], nan_quotient bool[nc], ids of v under c_prev); a: those ids, if already known."""
    v = np.asarray(v, F).reshape(-1)
    nc = c_prev.shape[0]
    if a is None:
        a = ro.kmeans_assign(v, c_prev)
    sizes = np.bincount(a, minlength=nc)
    with np.errstate(all="ignore"):
        sums = np.bincount(a, weights=v.astype(np.float64), minlength=nc).astype(F)
        want = (sums / sizes.astype(F)).astype(F)
    nanq = np.isnan(want)
    want[nanq] = 0
    return want, sizes, nanq, a


def bar(v, want, sizes):
    """The derived bar per centre (float64); only read where `want` is finite and the cluster is not empty."""
    v = np.asarray(v, F).reshape(-1)
    tot = np.abs(v[np.isfinite(v)].astype(np.float64)).sum()
    with np.errstate(all="ignore"):
        return 2.0 * ulp32(np.where(np.isfinite(want), want, 0)) + 2.0 ** -50 * tot / np.maximum(sizes, 1)


def check_update(got, v, c_prev, a=None):
    """Holds `got` (the centres after one more update than c_prev) to the oracle update; -> worst error / bar."""
    want, sizes, nanq, _ = oracle_update(v, c_prev, a)
    got = np.asarray(got, F)
    assert got.shape == want.shape and not np.isnan(got).any()
    exact = ~np.isfinite(want) | (sizes == 0) | nanq
    assert np.array_equal(got[exact], want[exact]), (
        f"infinite / empty / NaN->0 centres differ at {np.nonzero(exact & (got != want))[0][:8]}: "
        f"got {got[exact & (got != want)][:8]}, want {want[exact & (got != want)][:8]}")
    fin = ~exact
    assert np.isfinite(got[fin]).all(), f"centres {np.nonzero(fin & ~np.isfinite(got))[0][:8]} are not finite"
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    b = bar(v, want, sizes)[fin]
    ratio = float((err / b).max()) if err.size else 0.0
    worst = int(np.argmax(err / b)) if err.size else -1
    assert ratio <= 1.0, (f"centre {np.nonzero(fin)[0][worst]}: got {got[fin][worst]!r}, want {want[fin][worst]!r}, "
                          f"error {err[worst]:.3e} > bar {b[worst]:.3e}")
    return ratio


# ------------------------------------------------------------------------------------------------------- the shapes
def shape_values(n, nc):
    rng = np.random.default_rng(1000 * n + nc)
    return rng.normal(0, 1, n).astype(F)


def initial_centres(v, nc, seed=0):
    """Centres drawn from the (finite) values, plus -- from 4 centres on -- duplicates and centres that own nothing."""
    rng = np.random.default_rng(7919 * nc + v.shape[0] + seed)
    pool = v[np.isfinite(v) & (np.abs(v) < 1e30)]
    c = pool[rng.integers(0, pool.shape[0], nc)].astype(F).copy()
    if nc >= 4:
        c[nc - 1] = c[0]                              # a duplicate: the later index ends up empty
        c[nc // 2] = c[1]
        c[nc // 3] = F(np.abs(pool).max() * 2 + 1000)  # beyond every value by more than their range: owns nothing
    return c


def has_duplicates_and_empties(v, c):
    _, sizes, _, _ = oracle_update(v, c)
    return np.unique(c).shape[0] < c.shape[0] and bool((sizes == 0).any()) and bool((sizes > 0).any())


# --------------------------------------------------------------------------------------------------- the value sets
def _ascending(n, rng):
    return np.sort(rng.normal(0, 1, n).astype(F))


def _descending(n, rng):
    return _ascending(n, rng)[::-1].copy()


def _all_equal(n, rng):
    return np.full(n, 0.7, F)


def _two_values(n, rng):
    return rng.choice(np.array([-1.5, 2.25], F), n)


def _offset(n, rng):
    return (1000 + rng.normal(0, 1e-3, n)).astype(F)


def _wide(n, rng):
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F)


def _zeros_subnormals(n, rng):
    v = rng.normal(0, 1, n)
    kind = rng.integers(0, 5, n)
    v = np.where(kind == 1, v * 1e-40, v)            # subnormal
    v = np.where(kind == 2, v * 3e-45, v)            # the last few subnormals, many of them equal or +-0
    v = v.astype(F)
    v[kind == 3] = 0.0
    v[kind == 4] = -0.0
    return v


def _with(extra):
    def make(n, rng):
        v = rng.normal(0, 1, n).astype(F)
        at = rng.choice(n, len(extra), replace=False)
        v[at] = np.array(extra, F)
        return v
    return make


VALUE_SETS = {
    "ascending": _ascending,
    "descending": _descending,
    "all_equal": _all_equal,
    "two_values": _two_values,
    "offset_1000": _offset,
    "wide_range": _wide,
    "zeros_subnormals": _zeros_subnormals,
    "flt_max": _with([FLT_MAX] * 5),
    "pos_inf": _with([np.inf] * 4),
    "neg_inf": _with([-np.inf] * 3),
    "both_inf": _with([np.inf] * 3 + [-np.inf] * 2),
}


def set_values(name, n):
    return VALUE_SETS[name](n, np.random.default_rng(n + sum(map(ord, name))))


# ------------------------------------------------------------------------------------------------------- convergence
BLOB_TOL = 1e-6


def blobs():
    """Three tight, well-separated blobs and three centres of which two start in the first blob: the assignment
    changes over the first updates and is then stable whatever the last bit of a centre, so the number of updates
    until the shift is below BLOB_TOL (it becomes exactly 0) is the same for every correct implementation."""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.normal(-5, 0.01, 1000), rng.normal(0, 0.01, 1500), rng.normal(5, 0.01, 777)])
    return rng.permutation(v).astype(F), np.array([-5.2, -4.8, 6.0], F)


# -------------------------------------------------- the library's route to a sum, in numpy (the bar's CPU check)
def blocked_prefix(x, block=256):
    """Exclusive fp64 prefix [n + 1] of x the way a parallel scan forms it: sums inside a block start from 0 (sorted
    neighbours, comparable magnitudes), and an entry is a block's running offset plus the sum inside the block -- a few
    roundings at the prefix's magnitude per entry.  (One running sum over all values, np.cumsum, is NOT within the bar
    on the wide-range set: a value below half an ulp of the running sum is absorbed whole, thousands of times over.)"""
    n = x.shape[0]
    pad = np.zeros((n + block - 1) // block * block, np.float64)
    pad[:n] = x
    local = np.cumsum(pad.reshape(-1, block), axis=1)
    offs = np.concatenate([[0.0], np.cumsum(local[:, -1])[:-1]]) if local.shape[0] else np.zeros(0)
    return np.concatenate([[0.0], (local + offs[:, None]).reshape(-1)[:n]])


def prefix_difference_update(v, c_prev):
    """One update the way csrc/kmeans.hip forms it: values sorted, an fp64 prefix sum of them with the infinite ones
    entered as 0, a cluster's sum = sum over its runs of (prefix[end] - prefix[start]) in fp64, cluster 0 additionally
    receives -inf / +inf once if such values exist; rounded to fp32 once, divided by the fp32 size, NaN -> 0."""
    v = np.sort(np.asarray(v, F).reshape(-1))
    nc = c_prev.shape[0]
    a = ro.kmeans_assign(v, c_prev)
    fin = np.isfinite(v)
    prefix = blocked_prefix(np.where(fin, v, 0).astype(np.float64))
    sums = np.zeros(nc, np.float64)
    sizes = np.zeros(nc, np.int64)
    n = v.shape[0]
    run = np.where(fin, a, np.where(v < 0, -2, -3))   # the infinite head and tail are runs of their own
    starts = np.nonzero(np.concatenate([[True], run[1:] != run[:-1]]))[0] if n else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [n]])
    with np.errstate(all="ignore"):
        for s, e in zip(starts, ends):
            if run[s] >= 0:
                sums[run[s]] += prefix[e] - prefix[s]
                sizes[run[s]] += e - s
            else:
                sums[0] += -np.inf if run[s] == -2 else np.inf
                sizes[0] += e - s
        new = (sums.astype(F) / sizes.astype(F)).astype(F)
    new[np.isnan(new)] = 0
    return new
