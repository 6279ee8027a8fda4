"""`_C.kmeans_cuda` / `r3dgs_kmeans` (csrc/kmeans.hip) update by update: every edge of the segment pass (8 values per
thread, 2048 per workgroup, its float4 path and its tail path, the closing add, n = 0), centre counts either side of the
centre sort's power-of-two padding, value sets that stress the fp64 prefix (order, ties, a common offset, a wide range,
subnormals, FLT_MAX, infinities), the device-side convergence flag, and the carved workspace.

The cases, the one-update oracle and the derived bar are tests/kmeans_cases.py's (its docstring has the derivation);
tests/test_kmeans_cpu.py checks the cases' preconditions and the bar without a GPU.  Each test prints its worst
achieved error / bar (`pytest -s`); profiles/kmeans_gpu_tests.txt records those lines."""
import numpy as np
import pytest

from oracle import reduction_ops as ro
from tests import kmeans_cases as cases

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(v, c, tol, its):
    from diff_gaussian_rasterization import _C
    ids, cen, iters = _C.kmeans_cuda(_dev(v).view(-1, 1), _dev(c), tol, its, _want_iterations=True)
    ids, cen = ids.cpu().numpy(), cen.cpu().numpy()
    assert ids.shape == (v.shape[0], 1) and ids.dtype == np.int32 and cen.shape == c.shape and cen.dtype == np.float32
    return ids[:, 0], cen, int(iters)


def _check_three_updates(label, v, c0):
    """Updates 1, 2, 3 (tol = 0, so max_iterations = k runs k updates), each against one oracle update of the library's own
    centres after k - 1; the returned ids against the returned centres, bit for bit."""
    ids, prev, it = _run(v, c0, 0.0, 0)
    a_prev = ro.kmeans_assign(v, c0)
    assert it == 0 and np.array_equal(prev, c0) and np.array_equal(ids, a_prev)
    worst = 0.0
    for k in (1, 2, 3):
        ids, cen, it = _run(v, c0, 0.0, k)
        assert it == k                                 # tol is a strict <: tol = 0 never stops early
        worst = max(worst, cases.check_update(cen, v, prev, a_prev))
        a_prev = ro.kmeans_assign(v, cen)
        assert np.array_equal(ids, a_prev)
        prev = cen
    print(f"kmeans_gpu {label}: worst error / bar over updates 1-3 = {worst:.3g}")


@pytest.mark.parametrize("n,nc", cases.SHAPES)
def test_gpu_kmeans_update_shapes(n, nc):
    v = cases.shape_values(n, nc)
    c0 = cases.initial_centres(v, nc)
    if nc >= 4:
        assert cases.has_duplicates_and_empties(v, c0)
    _check_three_updates(f"shape n={n} centres={nc}", v, c0)


@pytest.mark.parametrize("nc", [1, 2, 63, 64, 65, 256, 257, 1024])
def test_gpu_kmeans_no_values(nc):
    """n = 0 with updates: every cluster is empty, so every centre becomes 0; the ids are empty."""
    c0 = np.linspace(-1, 1, nc).astype(np.float32) + np.float32(2)
    ids, cen, it = _run(np.zeros(0, np.float32), c0, 0.0, 3)
    assert ids.shape == (0,) and it == 3 and np.array_equal(cen, np.zeros(nc, np.float32))
    ids, cen, it = _run(np.zeros(0, np.float32), c0, 0.0, 0)
    assert ids.shape == (0,) and it == 0 and np.array_equal(cen, c0)


@pytest.mark.parametrize("n", cases.SET_SIZES)
@pytest.mark.parametrize("name", list(cases.VALUE_SETS))
def test_gpu_kmeans_update_value_sets(name, n):
    v = cases.set_values(name, n)
    c0 = cases.initial_centres(v, cases.SET_CENTRES)
    assert cases.has_duplicates_and_empties(v, c0)
    _check_three_updates(f"set {name} n={n} centres={cases.SET_CENTRES}", v, c0)


def test_gpu_kmeans_convergence_flag():
    """Three blobs, three centres: iterations_run is the oracle's; once converged the remaining launches are no-ops."""
    v, c0 = cases.blobs()
    _, o_cen, o_it = ro.kmeans(v, c0, cases.BLOB_TOL, 20)
    assert 1 < o_it < 20
    ids, cen, it = _run(v, c0, cases.BLOB_TOL, 20)
    assert it == o_it
    np.testing.assert_allclose(cen, o_cen, rtol=1e-6, atol=1e-7)
    assert np.array_equal(ids, ro.kmeans_assign(v, cen))
    ids_a, cen_a, it_a = _run(v, c0, cases.BLOB_TOL, it)
    ids_b, cen_b, it_b = _run(v, c0, cases.BLOB_TOL, it + 50)
    assert it_a == it_b == it
    assert np.array_equal(cen_a.view(np.int32), cen_b.view(np.int32)) and np.array_equal(ids_a, ids_b)
    assert np.array_equal(cen_a.view(np.int32), cen.view(np.int32)) and np.array_equal(ids_a, ids)
    assert _run(v, c0, cases.BLOB_TOL, it - 1)[2] == it - 1
    # tol = 0 is never reached, not even by a shift of exactly 0
    assert _run(v, c0, 0.0, it + 7)[2] == it + 7


@pytest.mark.parametrize("name", ["normal", "wide_range", "offset_1000"])
def test_gpu_kmeans_run_to_run_identical(name):
    """Bit-identical centres and ids run to run at 65 537 x 256 -- also where clusters have several runs of sorted values
    (wide_range: cluster 0 collects every value whose squared distance to all centres overflows; tiny values tie between
    many centres), whose prefix entries meet in an order that differs from run to run."""
    v = cases.shape_values(65537, 256) if name == "normal" else cases.set_values(name, 65537)
    c0 = cases.initial_centres(v, 256)
    for tol, its in ((0.0, 3), (1e-4, 40)):
        first = _run(v, c0, tol, its)
        for _ in range(3):
            again = _run(v, c0, tol, its)
            assert np.array_equal(first[0], again[0]) and first[2] == again[2]
            assert np.array_equal(first[1].view(np.int32), again[1].view(np.int32))


@pytest.mark.parametrize("case", ["shape", "both_inf"])
def test_gpu_kmeans_workspace_is_scratch(case):
    """Through the C ABI: the reported size is enough (a guard behind it stays untouched) and nothing relies on the
    workspace's contents (all bytes 0xFF: NaN as a float or double, negative as an integer)."""
    import torch
    from diff_gaussian_rasterization import _C
    if case == "shape":
        v = cases.shape_values(65537, 257)
        c0 = cases.initial_centres(v, 257)
    else:
        v = cases.set_values("both_inf", 4097)
        c0 = cases.initial_centres(v, cases.SET_CENTRES)
    n, nc, guard = v.shape[0], c0.shape[0], 4096
    want_ids, want_cen, want_it = _run(v, c0, 0.0, 3)
    size = int(_C._lib.r3dgs_kmeans_workspace_bytes(n, nc))
    assert size > 0
    ws = torch.full((size + guard,), 0xFF, dtype=torch.uint8, device="cuda")
    dv, dc = _dev(v), _dev(c0)
    ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cen = torch.full((nc,), float("nan"), dtype=torch.float32, device="cuda")
    iters = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = _C._lib.r3dgs_kmeans(n, nc, dv.data_ptr(), dc.data_ptr(), 0.0, 3, ids.data_ptr(), cen.data_ptr(),
                              iters.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc >= 0, _C._lib.r3dgs_last_error().decode()
    torch.cuda.synchronize()
    assert int(iters) == want_it == 3
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(cen.cpu().numpy().view(np.int32), want_cen.view(np.int32))
    assert bool((ws[size:] == 0xFF).all()), "the call wrote behind the size it reported"
