"""What tests/test_kmeans_gpu.py rests on, checked without a GPU:
  * the oracle's update (oracle/reduction_ops.py: kmeans_assign + float64 np.bincount) with infinite values against a
    literal per-value fp32 loop of what the reference's updateIdsCUDA / updateCentersCUDA and its host loop do (one
    256-value block, values added in index order; sum / size; NaN -> 0);
  * the preconditions of the GPU cases (they are conditions, not measurements);
  * the derived bar of tests/kmeans_cases.py, on a numpy evaluation of the library's route to a sum (differences of an
    fp64 prefix of the sorted values)."""
import numpy as np
import pytest

from oracle import reduction_ops as ro
from tests import kmeans_cases as cases

F = np.float32


def _literal_update(v, c):
    """One update, value by value in fp32: nearest centre by the first strictly smaller sqrt((c - v)^2) starting from
    inf at index 0, the value added to that centre's fp32 sum; then sum / size with NaN -> 0."""
    sums = [F(0)] * len(c)
    sizes = [0] * len(c)
    ids = []
    with np.errstate(all="ignore"):
        for x in v:
            best, at = F(np.inf), 0
            for i, ci in enumerate(c):
                t = F(F(ci) - F(x))
                d = F(np.sqrt(F(t * t)))
                if d < best:
                    best, at = d, i
            ids.append(at)
            sums[at] = F(sums[at] + F(x))
            sizes[at] += 1
        new = np.array([F(s) / F(k) for s, k in zip(sums, sizes)], F)
    new[np.isnan(new)] = 0
    return np.array(ids, np.int32), new


_INF_CASES = {
    "pos_inf": [np.inf, np.inf],
    "neg_inf": [-np.inf],
    "both_inf": [np.inf, -np.inf, -np.inf],
    "flt_max": [cases.FLT_MAX] * 3,
}


@pytest.mark.parametrize("name", list(_INF_CASES))
@pytest.mark.parametrize("n", [5, 64, 200])
def test_oracle_update_with_infinities_matches_the_literal_loop(name, n):
    rng = np.random.default_rng(n)
    extra = np.array(_INF_CASES[name], F)
    v = rng.normal(0, 1, n).astype(F)
    v[rng.choice(n, extra.shape[0], replace=False)] = extra
    fin = v[np.isfinite(v) & (np.abs(v) < 1e30)]
    c = fin[rng.integers(0, fin.shape[0], 6)].copy()
    c[4] = c[1]                                        # a duplicate: empty -> NaN -> 0
    ids, lit = _literal_update(v, c)
    want, sizes, nanq, a = cases.oracle_update(v, c)
    assert np.array_equal(a, ids)
    # an infinite value (and FLT_MAX, whose squared distance overflows) is nearer to no centre than the initial inf
    assert (ids[~np.isfinite(v) | (v == cases.FLT_MAX)] == 0).all()
    assert np.array_equal(np.isinf(want), np.isinf(lit)) and np.array_equal(want == 0, lit == 0)
    assert np.array_equal(want[np.isinf(want)], lit[np.isinf(lit)])            # the same sign
    ok = np.isfinite(want) & (want != 0)
    np.testing.assert_allclose(want[ok], lit[ok], rtol=1e-6)
    # the cluster that holds the special values is what the case says, and no other centre is touched by them
    expect0 = {"pos_inf": np.inf, "neg_inf": -np.inf, "both_inf": 0.0, "flt_max": np.inf}[name]
    assert want[0] == expect0 and (name != "both_inf" or nanq[0])
    assert np.isfinite(want[1:]).all() and want[4] == 0 and sizes[4] == 0
    # and the library's route (infinite values out of the prefix, added to cluster 0 on their own) says the same
    got = cases.prefix_difference_update(v, c)
    assert cases.check_update(got, v, c) <= 1.0


def test_bar_helpers():
    assert cases.ulp32(1.0) == 2.0 ** -23 and cases.ulp32(1.9999) == 2.0 ** -23 and cases.ulp32(2.0) == 2.0 ** -22
    assert cases.ulp32(0.0) == 2.0 ** -149 and cases.ulp32(1e-40) == 2.0 ** -149
    assert cases.ulp32(-3.0) == 2.0 ** -22 and cases.ulp32(float(cases.FLT_MAX)) == 2.0 ** 104
    # the checker refuses what the bar forbids: the poisoning a single -inf used to cause, a lost infinity, 3 ulp
    v = cases.set_values("neg_inf", 4097)
    c = cases.initial_centres(v, 16)
    want, sizes, _, _ = cases.oracle_update(v, c)
    assert want[0] == -np.inf and cases.check_update(want, v, c) == 0.0
    poisoned = want.copy()
    poisoned[1:] = 0
    with pytest.raises(AssertionError):
        cases.check_update(poisoned, v, c)
    lost = want.copy()
    lost[0] = 0
    with pytest.raises(AssertionError):
        cases.check_update(lost, v, c)
    k = int(np.argmax(sizes))
    off = want.copy()
    off[k] = np.nextafter(np.nextafter(np.nextafter(off[k], F(9)), F(9)), F(9))
    assert 2.0 ** -50 * np.abs(v[np.isfinite(v)]).sum() / sizes[k] < 0.5 * cases.ulp32(want[k])
    with pytest.raises(AssertionError):
        cases.check_update(off, v, c)


def test_shape_cases_cover_the_edges_and_have_duplicates_and_empty_clusters():
    assert {n for n, _ in cases.SHAPES} | {0} == {0, 1, 7, 8, 9, 2047, 2048, 2049, 4097, 65537}
    assert {nc for _, nc in cases.SHAPES} == {1, 2, 63, 64, 65, 256, 257, 1024}
    for n, nc in cases.SHAPES:
        if nc >= 4 and n * nc <= 2049 * 257:           # the larger ones are asserted where they run
            v = cases.shape_values(n, nc)
            assert cases.has_duplicates_and_empties(v, cases.initial_centres(v, nc)), (n, nc)


@pytest.mark.parametrize("n", cases.SET_SIZES)
@pytest.mark.parametrize("name", list(cases.VALUE_SETS))
def test_value_set_preconditions_and_bar(name, n):
    v = cases.set_values(name, n)
    assert v.dtype == F and v.shape == (n,) and not np.isnan(v).any()
    c0 = cases.initial_centres(v, cases.SET_CENTRES)
    assert np.isfinite(c0).all() and cases.has_duplicates_and_empties(v, c0)
    want, sizes, nanq, a = cases.oracle_update(v, c0)
    if name == "ascending":
        assert (np.diff(v) >= 0).all()
    if name == "descending":
        assert (np.diff(v) <= 0).all()
    if name == "all_equal":
        assert np.unique(v).shape[0] == 1 and (sizes > 0).sum() == 1
    if name == "two_values":
        assert np.unique(v).shape[0] == 2 and (sizes > 0).sum() == 2
    if name == "offset_1000":
        assert np.abs(v - 1000).max() < 0.01 and np.unique(v).shape[0] < 300   # few distinct fp32 values: midpoint ties
    if name == "wide_range":
        assert np.abs(v).max() > 1e29 and 0 < np.abs(v).min() < 1e-29
    if name == "zeros_subnormals":
        tiny = np.finfo(F).tiny
        assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
        assert ((v != 0) & (np.abs(v) < tiny)).sum() > n // 10
    if name == "flt_max":
        assert (v == cases.FLT_MAX).sum() == 5 and want[0] == np.inf and np.isfinite(want[1:]).all()
    if name == "pos_inf":
        assert (v == np.inf).sum() == 4 and want[0] == np.inf and np.isfinite(want[1:]).all()
    if name == "neg_inf":
        assert (v == -np.inf).sum() == 3 and want[0] == -np.inf and np.isfinite(want[1:]).all()
        assert (want[1:] != 0).sum() > 100             # what the poisoned prefix used to turn into 0
    if name == "both_inf":
        assert (v == np.inf).sum() == 3 and (v == -np.inf).sum() == 2 and nanq[0] and sizes[0] >= 5 and want[0] == 0
    # three updates along the library's route stay under the bar, each against the oracle on the same previous centres
    prev = c0
    for _ in range(3):
        got = cases.prefix_difference_update(v, prev)
        assert cases.check_update(got, v, prev) <= 1.0
        prev = got


def test_blobs_converge_in_fewer_than_20_updates():
    v, c0 = cases.blobs()
    ids, cen, it = ro.kmeans(v, c0, cases.BLOB_TOL, 20)
    assert 1 < it < 20
    assert sorted(np.bincount(ids[:, 0], minlength=3).tolist()) == [777, 1000, 1500]
    # stable: one more update moves nothing, so the count does not depend on a centre's last bit
    _, cen2, it2 = ro.kmeans(v, c0, cases.BLOB_TOL, 60)
    assert it2 == it and np.array_equal(cen, cen2)
    # and the first updates do change the assignment (the flag must not be set by them)
    _, c1, _ = ro.kmeans(v, c0, 0.0, 1)
    assert not np.array_equal(ro.kmeans_assign(v, c0), ro.kmeans_assign(v, c1))
