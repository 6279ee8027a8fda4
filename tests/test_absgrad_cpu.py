"""CPU checks of the absolute screen-space gradients (include/r3dgs_rasterizer.h r3dgs_backward_absgrad; csrc/blend_math.h
bwd_accumulate_abs): the float64 restatement tests/absgrad_ref.py pinned to oracle/backward_f64 and by its own invariants; the
device's accumulate run on the host (tests/hostcheck_absgrad) held to it; the seeded scenes of the GPU tests held inside the
ambiguity cap by the reference alone; the host surface (ABI rows, refusals, the statistics' error).  No GPU needed."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import synth_scene as ss
from oracle import oracle as orc
from tests import absgrad_ref as ag
from tests import camera_cases as cc
from tests import hostcheck_build as hb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-4                  # the project's gradient bar, relative to max|ref| per column
AMBIG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels (tests/test_gpu_parity.py)


def oracle_forward(cam, g, bg, W, H):
    return orc.forward(bg, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                       cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                       want_ambig=True, ambig_rel=1e-5)


def scene_list():
    out = []
    for name, kw in (("tiles", ag.SCENE_TILES), ("one_tile", ag.SCENE_ONE_TILE)):
        cam, g, bg = ag.make_scene(kw)
        out.append((name, cam, g, bg, kw["W"], kw["H"]))
    cam, g = cc.cloud(ag.PORTRAIT["camera"], "gpu", ag.PORTRAIT["P"], ag.PORTRAIT["seed"])
    out.append(("portrait", cam, g, np.array([0.1, 0.3, 0.2], np.float32), cam.image_width, cam.image_height))
    return out


@pytest.fixture(scope="module")
def scenes():
    """name -> (oracle forward, masked upstream gradient, absgrad_ref of it): computed once, left unchanged."""
    out = {}
    for k, (name, cam, g, bg, W, H) in enumerate(scene_list()):
        ref = oracle_forward(cam, g, bg, W, H)
        dl = ag.masked_upstream(ss.upstream_grad(W, H, seed=40 + k) * (W * H), ref["ambig"])
        out[name] = (ref, dl, ag.absgrad_ref(ref["state"], dl, ref["ambig"]))
    return out


def test_the_seeded_scenes_stay_inside_the_ambiguity_cap(scenes):
    for name, (ref, dl, r) in scenes.items():
        assert r["ambig"].mean() <= AMBIG_MAX_FRACTION, (name, r["ambig"].mean())
        assert (r["abs"] > 0).any(), name


def test_the_signed_column_is_the_oracles(scenes):
    """Pins the restatement: its signed sums are oracle/backward_f64's dL_dmean2D."""
    for name, (ref, dl, r) in scenes.items():
        want = orc.backward_f64(ref["state"], dl, 0.0)["dL_dmeans2D"][:, :2]
        scale = np.abs(want).max()
        assert scale > 0
        assert np.abs(r["signed"] - want).max() <= 1e-10 * scale, name


def test_abs_dominates_signed_exactly(scenes):
    for name, (ref, dl, r) in scenes.items():
        assert (r["abs"] >= np.abs(r["signed"])).all(), name
        assert (r["abs"] > np.abs(r["signed"])).any(), name   # somewhere the per-pixel terms do cancel
        culled = ref["state"]["radii"] <= 0
        assert not r["abs"][culled].any()


def test_one_pixel_image_has_one_term_per_gaussian():
    """A single pixel: each Gaussian has one term, so abs == |signed| exactly."""
    entries = [(0.4, -0.3, 0.5, 0.1, 0.7, 0.6), (-0.6, 0.2, 0.3, -0.05, 0.4, 0.8), (0.1, 0.9, 0.9, 0.2, 0.6, 0.5)]
    st = ag.hand_state(entries, [(0.9, 0.1, 0.3), (0.2, 0.8, 0.5), (0.4, 0.4, 0.9)], [3], bg=(0.1, 0.2, 0.3))
    dl = np.array([0.7, -1.3, 0.4], np.float32).reshape(3, 1, 1)
    r = ag.absgrad_ref(st, dl)
    assert (r["signed"] != 0).all()
    np.testing.assert_array_equal(r["abs"], np.abs(r["signed"]))


def test_the_device_accumulate_on_the_host_agrees(scenes):
    lib = hb.build_shim(os.path.join(ROOT, "tests", "hostcheck_absgrad", "hostcheck_absgrad.hip"),
                        os.path.join(ROOT, "tests", "hostcheck_absgrad", "libhostcheck_absgrad.so"),
                        ("-ffp-contract=fast",), "hipcc is needed to build the host check")
    for name, (ref, dl, r) in scenes.items():
        st = ref["state"]
        P, W, H = st["P"], st["W"], st["H"]

        def p(a, dt):
            a = np.ascontiguousarray(a, dtype=dt)
            return a, a.ctypes.data_as(C.c_void_p)
        keep = [p(st["ranges"], np.uint32), p(st["point_list"], np.uint32), p(st["bg"], np.float32), p(st["xy"], np.float32),
                p(st["conic_op"], np.float32), p(st["rgb"], np.float32), p(st["final_T"], np.float32),
                p(st["n_contrib"], np.uint32), p(dl, np.float32)]
        signed, absol = np.zeros((P, 2)), np.zeros((P, 2))
        lib.hc_absgrad(C.c_int(P), C.c_int(W), C.c_int(H), *[k[1] for k in keep], signed.ctypes.data_as(C.c_void_p),
                       absol.ctypes.data_as(C.c_void_p))
        for col in range(2):
            for got, want, what in ((absol, r["abs"], "abs"), (signed, r["signed"], "signed")):
                scale = np.abs(want[:, col]).max()
                err = np.abs(got[:, col] - want[:, col]).max()
                print(f"{name} {what}[{col}]: err / max|ref| = {err / scale:.2e}")
                assert err <= REL * scale, (name, what, col, err / scale)


# ---- the host surface ----------------------------------------------------------------------------------------------------

def test_abi_rows_and_argument_counts():
    from diff_gaussian_rasterization import _C
    rows = {name: row for _, group in _C._ABI.values() for name, row in group.items()}
    assert len(rows["r3dgs_backward"][1]) == 36 and len(rows["r3dgs_backward_params"][1]) == 36
    assert rows["r3dgs_backward_absgrad"][1][:36] == rows["r3dgs_backward"][1]
    assert rows["r3dgs_backward_params_absgrad"][1][:36] == rows["r3dgs_backward_params"][1]
    for name in ("r3dgs_backward_absgrad", "r3dgs_backward_params_absgrad"):
        assert rows[name][1][36:] == [C.c_void_p, C.c_void_p, C.c_size_t] and rows[name][0] is C.c_int
    assert rows["r3dgs_absgrad_workspace_floats"] == (C.c_size_t, [C.c_int])
    assert _C.has_absgrad()
    for R in (1, 63, 64, 65, 100000):
        assert _C._lib.r3dgs_absgrad_workspace_floats(R) == (R // 64 + 1) * 4
    listed = dict(_C._ext_loaded.entry_points())
    for name in _C._OPTIONAL_ROWS["absgrad"][1]:
        assert listed[name] is False   # optional for the compiled binding too


def test_an_older_library_loads_and_says_the_entry_points_are_absent(monkeypatch):
    from diff_gaussian_rasterization import _C
    names = _C._OPTIONAL_ROWS["absgrad"][1]
    lib = type("OlderLibrary", (), {})()
    for group, (_, rows) in _C._ABI.items():
        for name in rows:
            if name not in names:
                setattr(lib, name, type("Fn", (), dict(restype=None, argtypes=None))())
    assert _C._apply_abi(lib) == set(_C._ABI)   # every group is still there
    monkeypatch.setattr(_C, "_missing_rows", set(names))
    assert not _C.has_absgrad()
    with pytest.raises(RuntimeError, match="absolute-gradient entry points.*rebuild it with build.py"):
        _C._need_rows("absgrad")


def _refused(call, binning_at, *tail):
    """The abs entry point `call` with every other pointer NULL: the abs arguments are looked at first."""
    from diff_gaussian_rasterization import _C
    n = len(call.argtypes) - 3
    args = [0 if t is C.c_int else 0.0 if t is C.c_float else None for t in call.argtypes[:n]]
    args[0], args[3] = 5, 1000                       # P, R
    args[binning_at] = C.c_void_p(64)                # binning_buffer: "a pass with pairs" (never read: the call is refused)
    assert call(*args, *tail) == -1
    return _C._lib.r3dgs_last_error().decode()


def test_refusals_null_pointer_and_short_workspace():
    from diff_gaussian_rasterization import _C
    need = _C._lib.r3dgs_absgrad_workspace_floats(1000)
    # (binning_buffer is parameter 21 of r3dgs_backward and 20 of r3dgs_backward_params, which has one array less in front)
    for call, at in ((_C._lib.r3dgs_backward_absgrad, 21), (_C._lib.r3dgs_backward_params_absgrad, 20)):
        assert "dL_dmean2D_abs is NULL" in _refused(call, at, None, C.c_void_p(64), need)
        msg = _refused(call, at, C.c_void_p(64), C.c_void_p(64), need - 1)
        assert f"holds {need - 1} floats" in msg and str(need) in msg
        assert "holds 0 floats" in _refused(call, at, C.c_void_p(64), None, need)


def test_the_statistics_refuse_a_tensor_without_absgrad():
    import r3dgs_train_stats as ts
    assert list(inspect.signature(ts.add_densification_stats_absgrad).parameters) == ["pc", "viewspace_point_tensor", "radii"]
    with pytest.raises(RuntimeError, match="has no .absgrad"):
        ts.add_densification_stats_absgrad(object(), torch.zeros(4, 3, requires_grad=True), torch.zeros(4, dtype=torch.int32))


def test_the_python_surface():
    import diff_gaussian_rasterization as dgr
    import r3dgs_render
    assert "absgrad" in inspect.signature(dgr.rasterize_gaussians).parameters
    assert "absgrad" not in inspect.signature(r3dgs_render.render).parameters   # a keyword on top, like `aux`
    assert "absgrad" not in dgr.GaussianRasterizationSettings._fields
    with dgr.absgrad():
        assert dgr._absgrad_request.scope is True
        with dgr.absgrad(False):
            assert dgr._absgrad_request.scope is False
        assert dgr._absgrad_request.scope is True
    assert dgr._absgrad_request.scope is False
