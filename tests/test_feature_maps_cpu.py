"""CPU checks of the feature maps (include/r3dgs_features.h, csrc/feature_math.h): the float64 reference tests/feature_ref.py
pinned by tests/aux_grad_ref.py (F = z is the depth map and its gradients, F = 1 the alpha map) and by the oracle's colour
render over a black background; the shared forward and backward steps run on the host by the stand-alone program
tests/hostcheck_features/hostcheck_features.hip over hand-built lists and a seeded scene, plainly and under the host
sanitizers; the scenes of the GPU tests held inside the project's cap on flagged pixels; and the host surface.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aux_grad_ref as agr
from tests import aux_ref as ar
from tests import feature_ref as fr
from tests import hostcheck_build as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels
REL = 1e-4                 # the project's gradient bar: max err <= 1e-4 * max |ref| per tensor
GROUP = 16                 # feature_math.h kFeatGroup
BG = np.array([0.1, 0.3, 0.2], np.float32)


def oracle_state(kw, colors=None):
    cam, g, _ = ar.make_scene(kw)
    ref = orc.forward(np.zeros(3, np.float32) if colors is not None else BG, g["means3D"], colors, g["opacity"], g["scales"],
                      g["rotations"], 1.0, None, cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy,
                      kw["H"], kw["W"], None if colors is not None else g["sh"], g["degrees"], cam.camera_center, want_ambig=True)
    return cam, g, ref


@pytest.fixture(scope="module")
def scene_b():
    cam, g, ref = oracle_state(ar.SCENE_B)
    return cam, g, ref["state"], ref["ambig"].reshape(-1) == 0


def features_of(P, C, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (P, C)).astype(np.float32)


def test_depth_as_a_feature_reproduces_aux_grad_ref(scene_b):
    """F = z: the depth map of aux_grad_ref and all of its gradients, to 1e-12 relative; F = 1: the alpha map."""
    cam, g, st, ok = scene_b
    H, W = st["H"], st["W"]
    gD = np.random.default_rng(1).uniform(-1.0, 1.0, H * W) * ok
    args = (g["means3D"], g["opacity"], g["scales"], g["rotations"], cam.world_view_transform, cam.full_proj_transform,
            cam.tanfovx, cam.tanfovy)
    want = agr.reference_grads(st, *args, g_depth=gD)
    t = agr._t
    xy64, co64, z64 = agr.geometry(t(g["means3D"]), t(g["opacity"]), t(g["scales"]), t(g["rotations"]), t(cam.world_view_transform),
                                   t(cam.full_proj_transform), W, H, cam.tanfovx, cam.tanfovy)   # float64, as agr has them
    z = z64.numpy().reshape(-1, 1)
    # (z as a constant feature: aux_grad_ref's gradient through z itself is its `z` entry, which reaches means3D through the
    # view's third row; taken out below so that both sides differentiate the blend alone)
    got = fr.reference_grads(st, *args, z, gD[None, :])
    np.testing.assert_allclose(got["map"][0], want["maps"]["depth"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(got["features"][:, 0], want["z"], rtol=1e-12, atol=1e-300)
    V = np.asarray(cam.world_view_transform, np.float64).reshape(4, 4)
    through_z = want["z"][:, None] * V[:3, 2][None, :]
    scale = np.abs(want["means3D"]).max()
    np.testing.assert_allclose(got["means3D"] + through_z, want["means3D"], rtol=1e-12, atol=1e-12 * scale)
    for k in ("opacity", "scales", "rotations", "means2D"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-12 * np.abs(want[k]).max(), err_msg=k)
    import torch
    ones = fr.walk(st, xy64, co64, torch.ones(len(z), 1, dtype=torch.float64)).numpy()
    np.testing.assert_allclose(ones[0], want["maps"]["alpha"], rtol=1e-12, atol=1e-300)


def test_first_three_channels_are_a_colour_render_over_black():
    """oracle.forward(bg = 0, colors_precomp = F[:, :3]) within 1e-5 off the flagged pixels, on scene B."""
    kw = ar.SCENE_B
    F = np.abs(features_of(kw["P"], 5, 2))   # colours in [0, 1]
    _, _, ref = oracle_state(kw, colors=np.ascontiguousarray(F[:, :3]))
    ok = ref["ambig"].reshape(-1) == 0
    share = 1.0 - ok.mean()
    print(f"[feature maps scene B] oracle-ambiguous {100 * share:.4f} %")
    assert share <= FLAG_MAX_FRACTION
    got = fr.feature_map(ref["state"], F)
    err = np.abs(got[:3] - ref["color"].reshape(3, -1))[:, ok].max()
    print(f"[feature maps scene B] first three channels against the oracle's colour render: max err {err:.3e}")
    assert err <= 1e-5 * max(1.0, float(np.abs(F).max()))
    assert np.abs(got[:3]).max() > 0.1


def test_the_gpu_scenes_stay_inside_the_cap():
    from tests import camera_cases as cc
    scenes = {"A": oracle_state(ar.SCENE_A)[2], "B": oracle_state(ar.SCENE_B)[2]}
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", 600, ar.PORTRAIT["seed"])
    scenes["portrait_far"] = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None,
                                         cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy,
                                         cam.image_height, cam.image_width, g["sh"], g["degrees"], cam.camera_center, want_ambig=True)
    for name, ref in scenes.items():
        amb = float((ref["ambig"] != 0).mean())
        print(f"[feature maps scene {name}] oracle-ambiguous {100 * amb:.4f} %")
        assert amb <= FLAG_MAX_FRACTION, name
    lens = scenes["A"]["state"]["ranges"][:, 1].astype(np.int64) - scenes["A"]["state"]["ranges"][:, 0]
    assert lens.max() > 128, "scene A must have a list of two full staging chunks and a remainder"


def _build_hostcheck(name, extra):
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "tests", "hostcheck_features", "hostcheck_features.hip")
    exe = os.path.join(ROOT, "tests", "hostcheck_features", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hb._headers()):   # hostcheck_build's rule
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DR3_TRIP_FORMS_ON_HOST", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


def hand_states():
    """One-tile hand-built lists: a saturating stack, skipped entries among blended ones, an empty list."""
    def centred(op, x=5, y=9):
        return (x, y, 1.0, 0.0, 1.0, op, 1.0)
    return {"stack": ar.hand_state([centred(0.95) for _ in range(6)]),
            "skips": ar.hand_state([centred(0.3), centred(0.003), (6, 9, -1.0, 0.0, -1.0, 0.9, 1.0), centred(0.6, 8, 3),
                                    (3.5, 4.5, 0.2, 0.05, 0.1, 0.8, 1.0)]),
            "empty": ar.hand_state(np.zeros((0, 7)))}


def write_scene(path, st, F, g):
    W, H = int(st["W"]), int(st["H"])
    P, C = F.shape
    ranges, plist = np.asarray(st["ranges"]).reshape(-1, 2), np.asarray(st["point_list"]).reshape(-1)
    R = int(ranges[:, 1].max()) if len(ranges) else 0
    with open(path, "w") as f:
        f.write(f"{W} {H} {P} {R} {len(ranges)} {C}\n")
        f.write(" ".join(str(int(v)) for v in ranges.reshape(-1)) + "\n")
        f.write(" ".join(str(int(v)) for v in plist[:R]) + "\n")
        nc, fT = np.asarray(st["n_contrib"]).reshape(-1), np.asarray(st["final_T"], np.float32).reshape(-1)
        f.write("\n".join(f"{int(n)} {float(t)!r}" for n, t in zip(nc, fT)) + "\n")
        rows = np.concatenate([np.asarray(st["xy"], np.float32).reshape(P, 2), np.asarray(st["conic_op"], np.float32).reshape(P, 4)], 1)
        for a in (rows, F, g):
            f.write(" ".join(repr(float(v)) for v in np.asarray(a, np.float32).reshape(-1)) + "\n")
    return path


@pytest.fixture(scope="module")
def host_cases(scene_b, tmp_path_factory):
    """(state, F, g, reference) per case: the hand-built lists at C = 1 and a group plus one, scene B at C = 1, a whole group,
    a group plus one and three groups minus one.  g is zero on the oracle's flagged pixels."""
    d = tmp_path_factory.mktemp("features")
    _, _, st_b, ok_b = scene_b
    cases = {}
    todo = [(f"{name}-{C}", st, np.ones(st["W"] * st["H"], bool), C) for name, st in hand_states().items() for C in (1, GROUP + 1)]
    todo += [(f"B-{C}", st_b, ok_b, C) for C in (1, GROUP, GROUP + 1, 3 * GROUP - 1)]
    for k, (name, st, ok, C) in enumerate(todo):
        P = len(np.asarray(st["xy"]).reshape(-1, 2))
        F = features_of(P, C, 10 + k)
        g = np.random.default_rng(40 + k).uniform(-1.0, 1.0, (C, st["W"] * st["H"])).astype(np.float32) * ok[None, :]
        cases[name] = dict(P=P, C=C, path=write_scene(str(d / f"{name}.txt"), st, F, g), want=fr.state_grads(st, F, g))
    return cases


@pytest.mark.parametrize("name,extra", [("hostcheck_features", ()),
                                        ("hostcheck_features_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                                    "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_steps_on_the_host(host_cases, name, extra):
    """feature_math.h's forward and backward steps on the CPU: the program's own exactness and gamma checks, and its
    per-Gaussian gradients against the float64 reference at the project's gradient bar; the second build runs the host side
    under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    exe = _build_hostcheck(name, extra)
    for case, c in host_cases.items():
        out = subprocess.run([exe, c["path"]], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (case, out.stdout[-2000:] + out.stderr[-4000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        assert lines[-1].startswith("hostcheck_features: OK"), (case, lines[-1])
        if c["P"] == 0:
            continue
        got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[:-1]])
        assert got.shape == (c["P"], 6 + c["C"])
        want = c["want"]
        # splat_grad_of's conic B is the reference's convention (half the derivative of the off-diagonal term)
        cols = dict(xy=(got[:, 0:2], want["xy"]), conic=(got[:, 2:5] * np.array([1.0, 2.0, 1.0]), want["conic_op"][:, :3]),
                    opacity=(got[:, 5], want["conic_op"][:, 3]), features=(got[:, 6:], want["features"]))
        for k, (a, b) in cols.items():
            scale, err = np.abs(b).max(), np.abs(a - b).max()
            print(f"[hostcheck_features {case}] {k}: max err {err:.3e}, bar {REL * scale:.3e}")
            assert err <= REL * scale, (case, k, err, scale)
        assert np.abs(want["features"]).max() > 0 or case.startswith("empty")


def test_host_surface():
    import inspect

    import build
    import diff_gaussian_rasterization as dgr
    import r3dgs_render
    import torch
    from diff_gaussian_rasterization import _C
    assert build.UNITS["feature_maps.hip"] == build.UNITS["blend.hip"]
    rows = _C._ABI["required"][1]
    assert len(rows["r3dgs_feature_maps"][1]) == 11 and len(rows["r3dgs_feature_maps_backward"][1]) == 29
    assert len(rows["r3dgs_feature_maps_backward_workspace_bytes"][1]) == 5
    hdr = open(os.path.join(ROOT, "include", "r3dgs_features.h")).read()
    assert f"#define R3DGS_FEATURE_MAX_CHANNELS {_C.FEATURE_MAX_CHANNELS}" in hdr and _C.FEATURE_MAX_CHANNELS >= 256
    assert issubclass(dgr._FeatureMaps, torch.autograd.Function) and callable(dgr.feature_maps) and callable(dgr.feature_maps_backward)
    params = inspect.signature(r3dgs_render.render).parameters
    assert "features" not in params and "features_geom_grad" not in params   # keywords on top, like `aux`
    blobs = [torch.zeros(64, dtype=torch.uint8)] * 3
    for bad in (torch.zeros(4, 0), torch.zeros(4, _C.FEATURE_MAX_CHANNELS + 1), torch.zeros(3, 2), torch.zeros(4),
                torch.zeros(4, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="features|C ="):
            _C.feature_maps(4, 16, 16, 16, *blobs, bad)
    with pytest.raises(ValueError, match="unknown gradient"):
        _C.feature_maps_backward(4, 16, 16, 16, *blobs, None, None, 1.0, 1.0, None, None, 1.0, None, None, None, torch.zeros(4, 2),
                                 None, want=("normal",))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.feature_maps(4, 16, 16, 16, *blobs, torch.zeros(4, 2))
    with pytest.raises(ValueError, match="without features"):
        r3dgs_render.render(None, None, None, None, features_geom_grad=True)
    # the C entry points refuse a channel count outside the range by themselves, before they touch a pointer
    for C in (0, _C.FEATURE_MAX_CHANNELS + 1):
        assert _C._lib.r3dgs_feature_maps(0, 0, 16, 16, None, None, None, None, C, None, None) < 0
        assert b"channels" in _C._lib.r3dgs_last_error()
        assert _C._lib.r3dgs_feature_maps_backward_workspace_bytes(4, 16, C, 16, 16) == 0
