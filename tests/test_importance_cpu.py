"""CPU checks of the blend-contribution scores (include/r3dgs_importance.h, csrc/importance_math.h): the float64 reference
tests/importance_ref.py pinned by a hand-worked case, by the alpha map, by tests/feature_ref.py's dL_dF for C = 1 under an
all-ones gradient and by its own count of blended pairs; masking and scaling of the weight map; the shared step, the row
arithmetic and the per-Gaussian fold run on the host by the stand-alone program tests/hostcheck_importance/
hostcheck_importance.hip, plainly and under the host sanitizers; and the host surface.  No GPU needed."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import feature_ref as fr
from tests import hostcheck_build as hb
from tests import importance_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels
BG = np.array([0.1, 0.3, 0.2], np.float32)


def oracle_state(kw):
    cam, g, _ = ar.make_scene(kw)
    ref = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                      cam.full_proj_transform, cam.tanfovx, cam.tanfovy, kw["H"], kw["W"], g["sh"], g["degrees"], cam.camera_center,
                      want_ambig=True)
    return ref["state"], ref["ambig"].reshape(-1) != 0


@pytest.fixture(scope="module")
def scene_a():
    return oracle_state(ar.SCENE_A)


@pytest.fixture(scope="module")
def scene_b():
    st, amb = oracle_state(ar.SCENE_B)
    return st, amb, ir.scores_ref(st)


def test_hand_worked_case():
    """Two isotropic Gaussians (conic 1, 0, 1) on one tile of a 16x16 image: the front one at (4, 4) with opacity 0.75, the back
    one at (5, 4) with opacity 0.5.  alpha = o exp(-d^2 / 2) >= 1/255 <=> d^2 <= 2 ln(255 o): d^2 <= 10.51 for the front one --
    the 37 lattice points with dx^2 + dy^2 <= 10 -- and d^2 <= 9.69 for the back one, the 29 points with d^2 <= 9; all of them
    lie inside the image.  Nothing saturates (T >= 0.25 * 0.5).  0.75 and 0.5 are exact in fp32."""
    st = ar.hand_state([(4, 4, 1.0, 0.0, 1.0, 0.75, 1.0), (5, 4, 1.0, 0.0, 1.0, 0.5, 2.0)])
    got = ir.scores_ref(st)
    assert got["count"].tolist() == [37, 29]
    a0 = lambda x, y: 0.75 * math.exp(-0.5 * ((4 - x) ** 2 + (4 - y) ** 2)) if (4 - x) ** 2 + (4 - y) ** 2 <= 10 else 0.0   # noqa: E731
    s0 = sum(a0(x, y) for x in range(16) for y in range(16))
    s1 = sum(0.5 * math.exp(-0.5 * ((5 - x) ** 2 + (4 - y) ** 2)) * (1.0 - a0(x, y))
             for x in range(16) for y in range(16) if (5 - x) ** 2 + (4 - y) ** 2 <= 9)
    # the float32 inputs are exact here, so float64 agrees to rounding
    np.testing.assert_allclose(got["sum"], [s0, s1], rtol=1e-13)
    # the front one peaks at its centre with T = 1; the back one at its own centre (5, 4): 0.5 (1 - 0.75 e^-0.5) = 0.27255
    # (at (6, 4) it is 0.5 e^-0.5 (1 - 0.75 e^-2) = 0.27248)
    np.testing.assert_allclose(got["max"], [0.75, 0.5 * (1.0 - 0.75 * math.exp(-0.5))], rtol=1e-13)
    assert got["pairs"] == 66 and abs(got["alpha_total"] - (s0 + s1)) <= 1e-13 * (s0 + s1)
    # a region of interest: the column x = 6 alone, with weight 2
    m = np.zeros((16, 16), np.float32)
    m[:, 6] = 2.0
    roi = ir.scores_ref(st, m)
    assert roi["count"].tolist() == [5, 5]   # front: 4 + dy^2 <= 10 -> |dy| <= 2; back: 1 + dy^2 <= 9 -> |dy| <= 2
    np.testing.assert_allclose(roi["sum"][0], 2.0 * sum(a0(6, y) for y in range(16)), rtol=1e-13)
    np.testing.assert_allclose(roi["max"][0], 0.75 * math.exp(-2.0), rtol=1e-13)


def test_sum_over_gaussians_is_the_alpha_map(scene_b):
    """m = 1: every blended entry hands alpha T to exactly one Gaussian, and 1 - final T is their total per pixel.  Against the
    float64 alpha map (tests/feature_ref.py's walk of F = 1, which test_feature_maps_cpu pins to aux_grad_ref's alpha map) to
    1e-12 relative; tests/aux_ref.py's own alpha map is fp32, so it is met to fp32's precision."""
    st, _, got = scene_b
    P = len(st["xy"])
    alpha64 = fr.feature_map(st, np.ones((P, 1), np.float32))[0]
    total = float(got["sum"].sum())
    assert total > 100.0
    assert abs(total - alpha64.sum()) <= 1e-12 * alpha64.sum()
    assert abs(got["alpha_total"] - alpha64.sum()) <= 1e-12 * alpha64.sum()
    alpha32 = ar.aux_ref(st)["alpha"].astype(np.float64)
    assert abs(total - alpha32.sum()) <= 1e-6 * alpha32.sum()


def test_sum_is_the_feature_gradient_of_a_single_ones_channel(scene_a):
    """The workaround this unit replaces: dL_dF of feature_ref for C = 1 under an all-ones upstream gradient, on scene A."""
    st, _ = scene_a
    P, N = len(st["xy"]), st["W"] * st["H"]
    want = fr.state_grads(st, np.ones((P, 1), np.float32), np.ones((1, N), np.float32))["features"][:, 0]
    got = ir.scores_ref(st)
    assert want.max() > 1.0
    np.testing.assert_allclose(got["sum"], want, rtol=1e-12, atol=1e-12 * want.max())
    assert ((got["count"] == 0) == (got["sum"] == 0)).all() and ((got["count"] == 0) == (got["max"] == 0)).all()
    assert got["max"].max() <= 0.99 and got["max"].max() > 0.5


def test_counts_add_up_to_the_blended_pairs(scene_b):
    st, _, got = scene_b
    assert int(got["count"].sum()) == got["pairs"] > 1000
    # per pixel nothing is blended behind the forward's last contributor, and the last contributor is blended
    n = np.asarray(st["n_contrib"]).reshape(-1)
    assert got["pairs"] <= int(n.sum()) and got["pairs"] >= int((n > 0).sum())


def test_masking_and_scaling(scene_b):
    st, _, full = scene_b
    H, W = st["H"], st["W"]
    rng = np.random.default_rng(5)
    gone = rng.random(H * W) < 0.3
    m = np.where(gone, 0.0, 1.0).astype(np.float32)
    masked, only = ir.scores_ref(st, m), ir.scores_ref(st, 1.0 - m)
    # the two halves partition every Gaussian's terms
    assert (masked["count"] + only["count"] == full["count"]).all()
    np.testing.assert_allclose(masked["sum"] + only["sum"], full["sum"], rtol=1e-12, atol=1e-300)
    assert (np.maximum(masked["max"], only["max"]) == full["max"]).all()
    assert (masked["count"] < full["count"]).any()
    # a negative zero masks like a positive one
    neg = np.where(gone, -0.0, 1.0).astype(np.float32)
    assert np.signbit(neg[gone]).all()
    for k in ("sum", "max", "count"):
        assert (ir.scores_ref(st, neg)[k] == masked[k]).all(), k
    doubled = ir.scores_ref(st, 2.0 * m)
    assert (doubled["sum"] == 2.0 * masked["sum"]).all()
    assert (doubled["max"] == masked["max"]).all() and (doubled["count"] == masked["count"]).all()
    zero = ir.scores_ref(st, np.zeros(H * W, np.float32))
    assert not zero["sum"].any() and not zero["max"].any() and not zero["count"].any()


def test_the_gpu_scenes_stay_inside_the_cap(scene_a, scene_b):
    for name, amb in (("A", scene_a[1]), ("B", scene_b[1])):
        print(f"[importance scene {name}] oracle-ambiguous {100 * amb.mean():.4f} %")
        assert amb.mean() <= FLAG_MAX_FRACTION
    lens = scene_b[0]["ranges"][:, 1].astype(np.int64) - scene_b[0]["ranges"][:, 0]
    assert lens.max() >= 256 and int(np.asarray(scene_b[0]["n_contrib"]).max()) > 64


# ---- the host check -----------------------------------------------------------------------------------------------------
def _build_hostcheck(name, extra):
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "tests", "hostcheck_importance", "hostcheck_importance.hip")
    exe = os.path.join(ROOT, "tests", "hostcheck_importance", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hb._headers()):   # hostcheck_build's rule
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


def hand_states():
    def centred(op, x=5, y=9):
        return (x, y, 1.0, 0.0, 1.0, op, 1.0)
    return {"stack": ar.hand_state([centred(0.95) for _ in range(6)]),
            "skips": ar.hand_state([centred(0.3), centred(0.003), (6, 9, -1.0, 0.0, -1.0, 0.9, 1.0), centred(0.6, 8, 3),
                                    (3.5, 4.5, 0.2, 0.05, 0.1, 0.8, 1.0)]),
            "empty": ar.hand_state(np.zeros((0, 7)))}


def weights_of(st, seed, amb=None):
    """A map in [-1, 1] with positive and negative zeros, a whole quadrant of zeros (all-zero rows) and zeros on `amb`."""
    H, W = st["H"], st["W"]
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32)
    m[rng.random((H, W)) < 0.1] = 0.0
    m[rng.random((H, W)) < 0.1] = -0.0
    m[:8, :8] = 0.0
    if amb is not None:
        m[amb.reshape(H, W)] = 0.0
    return m


def write_scene(path, st, m, accumulate, tiles, held):
    W, H = int(st["W"]), int(st["H"])
    P = len(np.asarray(st["xy"]).reshape(-1, 2))
    ranges, plist = np.asarray(st["ranges"]).reshape(-1, 2), np.asarray(st["point_list"]).reshape(-1)
    R = int(ranges[:, 1].max()) if len(ranges) else 0
    with open(path, "w") as f:
        f.write(f"{W} {H} {P} {R} {len(ranges)} {int(accumulate)}\n")
        f.write(" ".join(str(int(v)) for v in ranges.reshape(-1)) + "\n")
        f.write(" ".join(str(int(v)) for v in plist[:R]) + "\n")
        nc = np.asarray(st["n_contrib"]).reshape(-1)
        f.write("\n".join(f"{int(n)} {float(w)!r}" for n, w in zip(nc, np.asarray(m, np.float32).reshape(-1))) + "\n")
        rows = np.concatenate([np.asarray(st["xy"], np.float32).reshape(P, 2), np.asarray(st["conic_op"], np.float32).reshape(P, 4)], 1)
        for i in range(P):
            f.write(" ".join(repr(float(v)) for v in rows[i]) + f" {int(tiles[i])} {float(held['sum'][i])!r} "
                    f"{float(held['max'][i])!r} {int(held['count'][i])} {int(held['views'][i])}\n")
    return path


@pytest.fixture(scope="module")
def host_cases(scene_b, tmp_path_factory):
    """Per case: the scene file and what the fold must leave.  The hand-built lists and scene B, each overwritten and
    accumulated onto held values; in scene B every seventh Gaussian is declared to have wanted one pair more than its run
    holds (the overflow rule: it contributes nothing)."""
    d = tmp_path_factory.mktemp("importance")
    st_b, amb_b, _ = scene_b
    cases = {}
    todo = [(name, st, None) for name, st in hand_states().items()] + [("B", st_b, amb_b)]
    for k, (name, st, amb) in enumerate(todo):
        P = len(np.asarray(st["xy"]).reshape(-1, 2))
        m = weights_of(st, 20 + k, amb)
        ref = ir.scores_ref(st, m)
        R = int(np.asarray(st["ranges"]).reshape(-1, 2)[:, 1].max())
        run = np.bincount(np.asarray(st["point_list"]).reshape(-1)[:R].astype(np.int64), minlength=P)[:P]
        tiles = run.copy()
        if name == "B":
            tiles[::7] += 1
        complete = tiles == run
        view = {k_: np.where(complete, ref[k_], 0) for k_ in ("sum", "max", "count")}
        rng = np.random.default_rng(60 + k)
        held = dict(sum=rng.uniform(-5.0, 5.0, P), max=rng.uniform(0.0, 0.5, P).astype(np.float32), count=rng.integers(0, 1000, P),
                    views=rng.integers(0, 9, P))
        for accumulate in (0, 1):
            if accumulate:
                want = dict(sum=held["sum"] + view["sum"], max=np.maximum(held["max"], view["max"]), count=held["count"] + view["count"],
                            views=held["views"] + (view["count"] > 0))
            else:
                want = dict(view, views=(view["count"] > 0).astype(np.int64))
            cases[f"{name}-{'accumulate' if accumulate else 'overwrite'}"] = dict(
                P=P, path=write_scene(str(d / f"{name}-{accumulate}.txt"), st, m, accumulate, tiles, held), want=want,
                view_count=view["count"], dropped=int((~complete & (ref["count"] > 0)).sum()))
    return cases


@pytest.mark.parametrize("name,extra", [("hostcheck_importance", ()),
                                        ("hostcheck_importance_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                                      "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_rows_and_fold_on_the_host(host_cases, name, extra):
    """importance_math.h's step, row arithmetic and fold on the CPU against the float64 reference at the GPU tests' bars: count
    and views exact, max within 1e-5, sum within 1e-5 * max(1, count) (weights in [-1, 1]).  The second build runs the host
    side under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    exe = _build_hostcheck(name, extra)
    assert host_cases["B-overwrite"]["dropped"] > 10, "the overflow rule must have something to drop"
    for case, c in host_cases.items():
        out = subprocess.run([exe, c["path"]], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (case, out.stdout[-2000:] + out.stderr[-4000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        assert lines[-1].startswith("hostcheck_importance: OK"), (case, lines[-1])
        if c["P"] == 0:
            continue
        got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[:-1]])
        assert got.shape == (c["P"], 4)
        want = c["want"]
        assert (got[:, 2] == want["count"]).all() and (got[:, 3] == want["views"]).all(), case
        err_max = np.abs(got[:, 1] - want["max"]).max()
        err_sum = (np.abs(got[:, 0] - want["sum"]) / np.maximum(1, c["view_count"])).max()
        print(f"[hostcheck_importance {case}] max err {err_max:.3e} (bar 1e-5), sum err / max(1, count) {err_sum:.3e} (bar 1e-5)")
        assert err_max <= 1e-5 and err_sum <= 1e-5, case


def test_host_surface():
    import build
    import diff_gaussian_rasterization as dgr
    import r3dgs_importance as ri
    import torch
    from diff_gaussian_rasterization import _C
    assert build.UNITS["importance.hip"] == build.UNITS["blend.hip"]
    rows = _C._ABI["required"][1]
    assert len(rows["r3dgs_contribution_scores"][1]) == 17 and len(rows["r3dgs_contribution_scores_workspace_bytes"][1]) == 4
    assert hasattr(_C._lib, "r3dgs_contribution_scores") and hasattr(_C._lib, "r3dgs_contribution_scores_workspace_bytes")
    assert ("r3dgs_contribution_scores", True) in _C._ext_loaded.entry_points()
    assert dgr.Scores._fields == ("sum", "max", "count", "views") and ri.Scores is dgr.Scores
    blobs = [torch.zeros(64, dtype=torch.uint8)] * 3
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.contribution_scores(4, 16, 16, 16, *blobs)
    with pytest.raises(ValueError, match="Scores"):
        dgr.contribution_scores(4, 16, 16, 16, *blobs, out=dict(sum=torch.zeros(4)))
    with pytest.raises(ValueError, match="accumulate"):
        _C.contribution_scores(0, 0, 16, 16, *blobs, accumulate=True)
    with pytest.raises(ValueError, match="names among"):
        _C.contribution_scores(0, 0, 16, 16, *blobs, out=dict(mean=torch.zeros(0)))
    with pytest.raises(RuntimeError, match="device tensor"):
        _C.contribution_scores(0, 0, 16, 16, *blobs, out=dict(sum=torch.zeros(0, dtype=torch.float64)))
    # the mask: refusals and the criteria, on host tensors (plain torch)
    s = dgr.Scores(torch.tensor([3.0, 0.0, 0.5, 2.0, 0.0], dtype=torch.float64), torch.tensor([0.9, 0.0, 0.01, 0.4, 0.0]),
                   torch.tensor([10, 0, 2, 7, 0]), torch.tensor([2, 0, 1, 2, 0], dtype=torch.int32))
    with pytest.raises(ValueError, match="criterion"):
        ri.low_contribution_mask(s)
    with pytest.raises(ValueError, match="keep_fraction"):
        ri.low_contribution_mask(s, keep_fraction=1.5)
    with pytest.raises(ValueError, match="Scores"):
        ri.low_contribution_mask((s.sum,), max_below=0.1)
    assert ri.low_contribution_mask(s, max_below=0.1).tolist() == [False, True, True, False, True]
    assert ri.low_contribution_mask(s, max_below=0.1, never_seen=False).tolist() == [False, False, True, False, False]
    assert ri.low_contribution_mask(s, sum_below=2.5).tolist() == [False, True, True, True, True]
    assert ri.low_contribution_mask(s, keep_fraction=0.4).tolist() == [False, True, True, False, True]
    assert ri.low_contribution_mask(s, keep_fraction=1.0, never_seen=False).tolist() == [False] * 5
    # the C entry points refuse bad sizes by themselves, before they touch a pointer
    assert _C._lib.r3dgs_contribution_scores(4, 16, 0, 16, None, None, None, None, None, None, None, None, 0, None, None, None, None) < 0
    assert b"width" in _C._lib.r3dgs_last_error()
    assert _C._lib.r3dgs_contribution_scores(0, 0, 16, 16, None, None, None, None, None, None, None, None, 2, None, None, None, None) < 0
    assert b"accumulate" in _C._lib.r3dgs_last_error()
    assert _C._lib.r3dgs_contribution_scores_workspace_bytes(0, 16, 16, 16) == 0
