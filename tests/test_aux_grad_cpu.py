"""CPU checks of the gradients through the auxiliary maps (include/r3dgs_aux.h r3dgs_aux_maps_backward, csrc/aux_math.h): the
float64 reference tests/aux_grad_ref.py pinned by hand cases with closed-form answers; the shared step and the per-Gaussian
chain run on the host by the stand-alone program tests/hostcheck_aux_grad/hostcheck_aux_grad.hip over a seeded scene, plainly
and under the host sanitizers, against that reference; the scenes of the GPU tests held inside the project's cap on flagged
pixels by the reference alone; and the host surface.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aux_grad_ref as agr
from tests import aux_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels
REL = 1e-4                 # the project's gradient bar: max err <= 1e-4 * max |ref| per tensor
PIX = 9 * 16 + 5           # pixel (5, 9) of the one-tile hand states


def centred(op, z, x=5, y=9):
    """An isotropic unit conic centred on pixel (x, y): G = 1 there, alpha = min(0.99, op)."""
    return (x, y, 1.0, 0.0, 1.0, op, z)


def one_hot(value=1.0):
    g = np.zeros(256)
    g[PIX] = value
    return g


def test_one_gaussian_over_a_pixel():
    """depth = z o, alpha = o at the centre: d depth / dz = o, d depth / do = z, d alpha / do = 1 = T_final / (1 - alpha)."""
    st = ar.hand_state([centred(0.6, 4.0)])
    d = agr.state_grads(st, g_depth=one_hot())
    np.testing.assert_allclose(d["depths"], [0.6], rtol=1e-6)
    np.testing.assert_allclose(d["conic_op"][0, 3], 4.0, rtol=1e-12)
    a = agr.state_grads(st, g_alpha=one_hot(2.0))
    np.testing.assert_allclose(a["conic_op"][0, 3], 2.0, rtol=1e-12)
    assert not a["depths"].any() and not d["xy"].any()   # at the centre the falloff is flat
    # off the centre, pixel (7, 9): alpha = o exp(-2), d alpha / d(mean x) = -alpha * A * dx with dx = x - px = -2
    g = np.zeros(256)
    g[9 * 16 + 7] = 1.0
    a = agr.state_grads(st, g_alpha=g)
    alpha = np.float64(np.float32(0.6)) * np.exp(-2.0)
    np.testing.assert_allclose(a["xy"][0], [2.0 * alpha, 0.0], rtol=1e-6, atol=1e-15)
    np.testing.assert_allclose(a["conic_op"][0, 0], -0.5 * 4.0 * alpha, rtol=1e-6)


def test_two_gaussians_the_suffix_term():
    """d depth / d alpha_0 = z_0 T_0 - z_1 alpha_1 T_1 / (1 - alpha_0) = 2 - 3 * 0.3 = 1.1;  d depth / d alpha_1 = z_1 T_1 = 2.1;
    d alpha / d alpha_k = T_final / (1 - alpha_k) = 0.7 for both."""
    st = ar.hand_state([centred(0.3, 2.0), centred(0.3, 3.0)])
    d = agr.state_grads(st, g_depth=one_hot())
    np.testing.assert_allclose(d["conic_op"][:, 3], [1.1, 2.1], rtol=1e-6)
    np.testing.assert_allclose(d["depths"], [0.3, 0.3 * 0.7], rtol=1e-6)
    a = agr.state_grads(st, g_alpha=one_hot())
    np.testing.assert_allclose(a["conic_op"][:, 3], [0.7, 0.7], rtol=1e-6)


def test_saturated_pixel_stops_at_n_contrib():
    """T = 0.05, 0.0025, 1.25e-4, then the stop: entries 3, 4, 5 get nothing."""
    st = ar.hand_state([centred(0.95, 1.0 + k) for k in range(6)])
    assert st["n_contrib"][PIX] == 3
    r = agr.state_grads(st, g_depth=one_hot(), g_alpha=one_hot(), g_median=one_hot())
    assert r["conic_op"][:3, 3].all() and not r["conic_op"][3:].any() and not r["depths"][3:].any()
    np.testing.assert_allclose(r["depths"][:3], [0.95 + 1.0, 0.95 * 0.05, 0.95 * 0.0025], rtol=1e-6)   # the median is entry 0


def test_skipped_entries_contribute_nothing():
    plain = agr.state_grads(ar.hand_state([centred(0.3, 2.0), centred(0.3, 3.0)]), g_depth=one_hot(), g_alpha=one_hot(0.5))
    for skipped in (centred(0.003, 100.0), (6, 9, -1.0, 0.0, -1.0, 0.9, 100.0)):   # alpha < 1/255; power > 0
        r = agr.state_grads(ar.hand_state([centred(0.3, 2.0), skipped, centred(0.3, 3.0)]), g_depth=one_hot(), g_alpha=one_hot(0.5))
        for k in ("xy", "conic_op", "depths"):
            assert not r[k][1].any(), k
            np.testing.assert_array_equal(r[k][[0, 2]], plain[k])


def test_median_routes_to_exactly_one_depth():
    st = ar.hand_state([centred(0.3, 2.0), centred(0.3, 3.0), centred(0.3, 5.0)])   # T = 0.7, 0.49, 0.343: the second entry
    r = agr.state_grads(st, g_median=one_hot(3.0))
    np.testing.assert_array_equal(r["depths"], [0.0, 3.0, 0.0])
    assert not r["conic_op"].any() and not r["xy"].any()
    assert r["maps"]["median_depth"][PIX] == 3.0
    none = agr.state_grads(ar.hand_state([centred(0.3, 2.0)]), g_median=one_hot())   # T stays above 0.5: nobody is selected
    assert not none["depths"].any()


def test_empty_pixel():
    st = ar.hand_state([centred(0.9, 4.0)])
    g = np.zeros(256)
    g[15] = 1.0   # pixel (15, 0): alpha = 0.9 exp(-0.5 * 181) < 1/255
    r = agr.state_grads(st, g_depth=g, g_alpha=g, g_median=g)
    assert not r["xy"].any() and not r["conic_op"].any() and not r["depths"].any()
    r = agr.state_grads(ar.hand_state(np.zeros((0, 7))), g_depth=np.ones(256))
    assert r["depths"].shape == (0,)


def oracle_state(cam, g, H, W):
    ref = orc.forward(np.array([0.1, 0.3, 0.2], np.float32), g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None,
                      cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"],
                      cam.camera_center, want_ambig=True)
    return ref, ar.aux_ref(ref["state"])


def test_the_gpu_scenes_stay_inside_the_cap():
    """Measured over the reference's lists (printed): every scene of tests/test_aux_grad_gpu.py leaves at most 0.1 % of its
    pixels flagged, threshold-ambiguous and median-ambiguous each."""
    from tests import camera_cases as cc
    from tests.test_aux_grad_gpu import stacked
    scenes = {"A": ar.make_scene(ar.SCENE_A)[:2] + (ar.SCENE_A["H"], ar.SCENE_A["W"]),
              "17x17": ar.make_scene(ar.SCENE_17)[:2] + (17, 17)}
    cam, g = cc.cloud(ar.PORTRAIT["camera"], "gpu", 600, ar.PORTRAIT["seed"])
    scenes["portrait_far"] = (cam, g, cam.image_height, cam.image_width)
    for P in (512, 203):
        scenes[f"stacked {P}"] = stacked(P) + (32, 32)
    for name, (cam, g, H, W) in scenes.items():
        ref, a = oracle_state(cam, g, H, W)
        amb, med = float((ref["ambig"] != 0).mean()), float(a["median_ambig"].mean())
        print(f"[aux grad scene {name}] oracle-ambiguous {100 * amb:.4f} %, median-ambiguous {100 * med:.4f} %")
        assert amb <= FLAG_MAX_FRACTION and med <= FLAG_MAX_FRACTION, name
        if name.startswith("stacked"):   # a list of three chunks (512) / of two with a partial one (203)
            lens = ref["state"]["ranges"][:, 1] - ref["state"]["ranges"][:, 0]
            assert lens.max() > (128 if name.endswith("512") else 64), name


def _build_hostcheck(name, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "tests", "hostcheck_aux_grad", "hostcheck_aux_grad.hip")
    exe = os.path.join(ROOT, "tests", "hostcheck_aux_grad", name)
    hdrs = [os.path.join(ROOT, "reduced-3dgs_amd", "csrc", h) for h in ("aux_math.h", "blend_math.h", "gauss_math.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    """SCENE_17 (P = 300, 17x17: two tiles a side, one pixel wide at the edge), its oracle state, seeded upstream gradients
    (zero on flagged pixels), the reference, and the scene file of the host program."""
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    H, W, P = kw["H"], kw["W"], kw["P"]
    ref, a = oracle_state(cam, g, H, W)
    st = ref["state"]
    ok = ~((ref["ambig"].reshape(-1) != 0) | a["median_ambig"].reshape(-1))
    rng = np.random.default_rng(5)
    ups = [rng.uniform(-1.0, 1.0, H * W).astype(np.float32) * ok for _ in range(3)]
    want = agr.reference_grads(st, g["means3D"], g["opacity"], g["scales"], g["rotations"], cam.world_view_transform,
                               cam.full_proj_transform, cam.tanfovx, cam.tanfovy, *ups)
    ranges, plist = np.asarray(st["ranges"]).reshape(-1, 2), np.asarray(st["point_list"]).reshape(-1)
    R = int(ranges[:, 1].max()) if len(ranges) else 0

    def write(path, f64):
        with open(path, "w") as f:
            f.write(f"{W} {H} {P} {R} {len(ranges)} {int(f64)} {cam.tanfovx!r} {cam.tanfovy!r} 1.0\n")
            for m in (cam.world_view_transform, cam.full_proj_transform):
                f.write(" ".join(repr(float(v)) for v in np.asarray(m, np.float32).reshape(-1)) + "\n")
            f.write(" ".join(str(int(v)) for v in ranges.reshape(-1)) + "\n")
            f.write(" ".join(str(int(v)) for v in plist[:R]) + "\n")
            for k in range(H * W):
                f.write(f"{int(st['n_contrib'][k])} {float(st['final_T'][k])!r} {float(ups[0][k])!r} {float(ups[1][k])!r} {float(ups[2][k])!r}\n")
            for i in range(P):
                row = [int(st["radii"][i])] + [float(v) for v in st["xy"][i]] + [float(v) for v in st["conic_op"][i]] + \
                      [float(st["depths"][i])] + [float(v) for v in g["means3D"][i]] + [float(v) for v in g["scales"][i]] + \
                      [float(v) for v in g["rotations"][i]]
                f.write(" ".join(repr(v) for v in row) + "\n")
        return path
    d = tmp_path_factory.mktemp("aux_grad")
    return dict(P=P, want=want, files={f64: write(str(d / f"scene_{int(f64)}.txt"), f64) for f64 in (True, False)})


@pytest.mark.parametrize("name,extra", [("hostcheck_aux_grad", ()),
                                        ("hostcheck_aux_grad_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                                    "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_step_and_chain_on_the_host(host_scene, name, extra):
    """aux_math.h's step and chain on the CPU, in the device pass's order of summation, against the float64 reference at the
    project's gradient bar, with the chain in double and in fp32; the second build runs the host side under AddressSanitizer
    and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    exe = _build_hostcheck(name, extra)
    want = host_scene["want"]
    for f64, path in host_scene["files"].items():
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        assert lines[-1].startswith("hostcheck_aux_grad: OK")
        got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[:-1]])
        assert got.shape == (host_scene["P"], 14)
        cols = dict(means2D=got[:, 0:2], means3D=got[:, 2:5], opacity=got[:, 5:6], scales=got[:, 6:9], rotations=got[:, 9:13],
                    z=got[:, 13])
        for k, a in cols.items():
            b = np.asarray(want[k]).reshape(a.shape)
            scale, err = np.abs(b).max(), np.abs(a - b).max()
            print(f"[hostcheck_aux_grad f64={f64}] {k}: max err {err:.3e}, bar {REL * scale:.3e}")
            assert scale > 0 and err <= REL * scale, (k, f64, err, scale)


def test_host_surface():
    import inspect

    import build
    import diff_gaussian_rasterization as dgr
    import r3dgs_render
    import torch
    from diff_gaussian_rasterization import _C
    assert build.UNITS["aux_bwd.hip"] == build.UNITS["blend.hip"]
    rows = _C._ABI["required"][1]
    assert len(rows["r3dgs_aux_maps_backward"][1]) == 28 and len(rows["r3dgs_aux_maps_backward_workspace_bytes"][1]) == 4
    listed = dict(_C._ext_loaded.entry_points())
    assert listed["r3dgs_aux_maps_backward"] and listed["r3dgs_aux_maps_backward_workspace_bytes"]
    assert _C.AUX_GRADS == ("means2D", "means3D", "opacity", "scales", "rotations", "cov3D")
    assert issubclass(dgr._AuxMaps, torch.autograd.Function) and callable(dgr.aux_maps_backward)
    assert "aux_grad" not in inspect.signature(r3dgs_render.render).parameters   # a keyword on top, like `aux`
    with pytest.raises(ValueError, match="unknown gradient"):
        _C.aux_maps_backward(4, 16, 16, 16, *[torch.zeros(64, dtype=torch.uint8)] * 3, None, None, 1.0, 1.0, torch.zeros(4, 3), None,
                             1.0, None, None, None, want=("normal",))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.aux_maps_backward(4, 16, 16, 16, *[torch.zeros(64, dtype=torch.uint8)] * 3, torch.eye(4), torch.eye(4), 1.0, 1.0,
                              torch.zeros(4, 3), torch.ones(4, 3), 1.0, torch.zeros(4, 4), None, torch.ones(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="without aux"):
        r3dgs_render.render(None, None, None, None, aux_grad=True)
    with pytest.raises(ValueError, match="no_grad"), torch.no_grad():
        r3dgs_render.render(None, None, None, None, aux=("depth",), aux_grad=True)
