"""CPU checks of the surface-normal unit (reduced-3dgs_amd/r3dgs_normals.py, csrc/normals.hip, csrc/normal_math.h,
include/r3dgs_normals.h): the per-element kernel arithmetic runs on the host through a test shim and is held to the float64
restatement tests/normals_ref.py -- values and every partial derivative, no element masked (the reference file asserts the
margins of every case); the axis against the oracle's 3D covariance; planes with their analytic normals; the pixel-centre
convention against ndc2pix; the shim as a stand-alone program, plain and under ASan/UBSan; the ABI rows, every refusal, and
render()'s keyword handling with a fake model and no launch.  No GPU needed."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import hostcheck_build as hb
from tests import normals_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_normals", "hostcheck_normals.hip")
SO = os.path.join(HERE, "hostcheck_normals", "libhostcheck_normals.so")
F32 = np.float32
VALUE_BAR, GRAD_BAR = 1e-5, 1e-4   # the GPU tests' bars
SIZES = ((3, 3), (2, 5), (16, 16), (37, 29), (64, 48))   # (W, H): one interior pixel, all border, ragged tiles


def _shim():
    lib = hb.build_shim(SRC, SO, hb.EXACT, "hipcc not available to build the surface-normal host-check shim")
    vp, f, i = C.c_void_p, C.c_float, C.c_int
    lib.hc_normal_axis.argtypes, lib.hc_normal_axis.restype = [vp], i
    lib.hc_ndc2pix.argtypes, lib.hc_ndc2pix.restype = [f, i], f
    lib.hc_ray.argtypes = [i, i, f, f, i, i, vp]
    lib.hc_gaussian_normals.argtypes = [i, vp, vp, vp, i, vp, vp, vp]
    lib.hc_gaussian_normals_bwd.argtypes = [i, vp, vp, vp, i, vp, vp, vp, vp]
    lib.hc_depth_normal.argtypes = [i, i, f, f, vp, vp, vp, vp, i, vp, vp]
    lib.hc_depth_normal_bwd.argtypes = [i, i, f, f, vp, vp, vp, vp, i, f, vp, vp, vp, vp]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- references shared by the host and the GPU tests, computed once per case, never modified ------------------------------------

_CACHE = {}


def ref_gaussians(P, raw):
    """-> (case, g [P,3], normals, d_rot) of the float64 restatement; the margins are asserted here."""
    key = ("g", P, raw)
    if key not in _CACHE:
        g = ref.gaussians(P, seed=P)
        ref.check_margins_gaussians(g, raw)
        up = np.random.default_rng(P).normal(0, 1, (P, 3)).astype(F32)
        q = ref._t(g["rotation_raw" if raw else "rotations"]).requires_grad_(True)
        n = ref.gaussian_normals(ref._t(g["means3D"]), ref._t(g["scaling_raw" if raw else "scales"]), q, ref._t(g["viewmatrix"]),
                                 ref._t(g["campos"]), raw=raw)
        d_rot, = torch.autograd.grad((n * ref._t(up)).sum(), q)
        _CACHE[key] = (g, up, n.detach().numpy(), d_rot.numpy())
    return _CACHE[key]


def ref_image(W, H, use_alpha, use_weight, scale_by_alpha, loss=True):
    """-> (case, values, gradients) of the float64 restatement for one image size and one combination of options."""
    key = ("i", W, H, use_alpha, use_weight, scale_by_alpha, loss)
    if key not in _CACHE:
        im = ref.image(H, W, seed=W * 100 + H)
        depth = im["depth"] if use_alpha else im["z_only"]
        ref.check_margins_image(depth, im["alpha"] if use_alpha else None)
        d = ref._t(depth).requires_grad_(True)
        a = ref._t(im["alpha"]).requires_grad_(True) if use_alpha else None
        if loss:
            N = ref._t(im["normal_map"]).requires_grad_(True)
            L, surf = ref.normal_consistency(N, d, a, ref.TAN_FOVX, ref.TAN_FOVY, scale_by_alpha, ref._t(im["weight"]) if use_weight else None)
            leaves = [d, N] + ([a] if use_alpha else [])   # (an image that is all border depends on none of them)
            grads = torch.autograd.grad(L, leaves, allow_unused=True)
            grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
            out = dict(loss=float(L.detach()),surf=surf.detach().numpy(), d_depth=grads[0].numpy(), d_normal=grads[1].numpy())
        else:
            surf = ref.depth_to_normal(d, a, ref.TAN_FOVX, ref.TAN_FOVY)
            leaves = [d] + ([a] if use_alpha else [])   # (an image that is all border depends on none of them)
            grads = torch.autograd.grad((surf * ref._t(im["g_surf"])).sum(), leaves, allow_unused=True) if surf.requires_grad else [None] * len(leaves)
            grads = [torch.zeros_like(d) if g is None else g for g in grads]
            out = dict(surf=surf.detach().numpy(), d_depth=grads[0].numpy())
        if use_alpha:
            out["d_alpha"] = grads[-1].numpy()
        _CACHE[key] = (im, depth, out)
    return _CACHE[key]


def hold(got, want, what, figures=None):
    """Values within 1e-5 absolute, every gradient tensor within 1e-4 * max|ref| -> the figures, for the profile."""
    worst = {}
    for k, w in want.items():
        a = np.asarray(got[k], np.float64).reshape(np.shape(w))
        err = float(np.abs(a - w).max()) if np.size(w) else 0.0
        if k.startswith("d_"):
            top = float(np.abs(w).max()) if np.size(w) else 0.0
            worst[k] = err / top if top > 0 else err
            assert err <= GRAD_BAR * top + 1e-300, f"{what}: {k}: error {err:.3g}, bar {GRAD_BAR} * {top:.3g}"
        else:
            worst[k] = err
            assert err <= VALUE_BAR, f"{what}: {k}: error {err:.3g}, bar {VALUE_BAR}"
    line = f"normals: {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
    print(line)
    if figures is not None:
        figures.append(line)
    return worst


# ---- normal_math.h on the host: Gaussians ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("P", [1, 63, 1000])
def test_gaussian_normals_values_and_gradients_on_the_host(P, raw):
    lib = _shim()
    g, up, want_n, want_dq = ref_gaussians(P, raw)
    n, dq = np.zeros((P, 3), F32), np.zeros((P, 4), F32)
    sc, rot = g["scaling_raw" if raw else "scales"], g["rotation_raw" if raw else "rotations"]
    lib.hc_gaussian_normals(P, _p(g["means3D"]), _p(sc), _p(rot), int(raw), _p(g["viewmatrix"]), _p(g["campos"]), _p(n))
    lib.hc_gaussian_normals_bwd(P, _p(g["means3D"]), _p(sc), _p(rot), int(raw), _p(g["viewmatrix"]), _p(g["campos"]), _p(up), _p(dq))
    hold(dict(normals=n, d_rot=dq), dict(normals=want_n, d_rot=want_dq), f"host, gaussians P={P} raw={raw}")
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-5
    if P == 1000:
        assert set(np.argmin(g["scales"], axis=1)) == {0, 1, 2}, "every axis is picked somewhere"


def test_axis_is_the_eigenvector_of_the_oracle_covariance_and_faces_the_camera():
    """Sigma n = s_min^2 n for the 3D covariance the oracle computes from the same scales and rotation (a transposed R fails
    this), and the returned normal faces the camera: n_view . mean_view < 0."""
    from oracle import oracle as orc
    from tests import aux_ref as ar
    lib = _shim()
    kw = ar.SCENE_B
    cam, g, bg = ar.make_scene(kw)
    st = orc.forward(bg, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                     cam.full_proj_transform, cam.tanfovx, cam.tanfovy, kw["H"], kw["W"], g["sh"], g["degrees"], cam.camera_center)["state"]
    seen = np.flatnonzero(st["radii"] > 0)
    assert len(seen) > 100
    P = len(g["means3D"])
    sc, rot = np.ascontiguousarray(g["scales"], F32), np.ascontiguousarray(g["rotations"], F32)
    s2 = np.sort(sc.astype(np.float64), axis=1)
    apart = (s2[:, 1] - s2[:, 0]) >= 1e-2 * s2[:, 1]   # an eigenvector is only defined where the smallest eigenvalue is simple
    eye, far = np.eye(4, dtype=F32), np.array([1e6, 2e6, -3e6], F32)
    n_w = np.zeros((P, 3), F32)   # identity view: the world-frame axis, up to its sign
    lib.hc_gaussian_normals(P, _p(np.ascontiguousarray(g["means3D"], F32)), _p(sc), _p(rot), 0, _p(eye), _p(far), _p(n_w))
    c6 = st["cov3D"].astype(np.float64)
    checked = 0
    for i in seen[apart[seen]]:
        S = np.array([[c6[i, 0], c6[i, 1], c6[i, 2]], [c6[i, 1], c6[i, 3], c6[i, 4]], [c6[i, 2], c6[i, 4], c6[i, 5]]])
        assert np.abs(S @ n_w[i] - s2[i, 0] ** 2 * n_w[i]).max() <= 1e-5 * np.abs(S).max(), i
        checked += 1
    assert checked > 100
    # facing: in a seeded case's own view, where the margins are asserted
    g2, _, _, _ = ref_gaussians(1000, False)
    n = np.zeros((1000, 3), F32)
    lib.hc_gaussian_normals(1000, _p(g2["means3D"]), _p(g2["scales"]), _p(g2["rotations"]), 0, _p(g2["viewmatrix"]), _p(g2["campos"]), _p(n))
    m_view = np.concatenate([g2["means3D"], np.ones((1000, 1), F32)], 1).astype(np.float64) @ g2["viewmatrix"].astype(np.float64)
    assert ((n * m_view[:, :3]).sum(1) < 0).all(), "a normal looks away from the camera"


def test_a_tie_picks_the_lowest_index():
    lib = _shim()
    for s, k in (((1, 1, 1), 0), ((2, 1, 1), 1), ((1, 2, 1), 0), ((3, 2, 1), 2), ((1, 1, 0.5), 2), ((-3, -3, -2), 0)):
        a = np.array(s, F32)
        assert lib.hc_normal_axis(_p(a)) == k, s
        assert int(torch.argmin(torch.tensor(s, dtype=torch.float64))) == k, "the reference's argmin agrees"


# ---- normal_math.h on the host: images ------------------------------------------------------------------------------------------

def _host_image(lib, im, depth, W, H, use_alpha, use_weight, scale_by_alpha, loss):
    alpha = im["alpha"] if use_alpha else None
    N, w = (im["normal_map"], im["weight"] if use_weight else None) if loss else (None, None)
    surf, L = np.zeros((3, H, W), F32), C.c_double(0.0)
    lib.hc_depth_normal(H, W, ref.TAN_FOVX, ref.TAN_FOVY, _p(depth), _p(alpha), _p(N), _p(w), int(scale_by_alpha), _p(surf), C.byref(L))
    dd, da, dn = np.zeros((H, W), F32), np.zeros((H, W), F32), np.zeros((3, H, W), F32)
    lib.hc_depth_normal_bwd(H, W, ref.TAN_FOVX, ref.TAN_FOVY, _p(depth), _p(alpha), _p(N), _p(w), int(scale_by_alpha), 1.0,
                            None if loss else _p(im["g_surf"]), _p(dd), _p(da) if use_alpha else None, _p(dn) if loss else None)
    got = dict(surf=surf, d_depth=dd)
    if loss:
        got.update(loss=L.value, d_normal=dn)
    if use_alpha:
        got["d_alpha"] = da
    return got


@pytest.mark.parametrize("scale_by_alpha", [True, False])
@pytest.mark.parametrize("use_weight", [False, True])
@pytest.mark.parametrize("use_alpha", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_consistency_loss_values_and_gradients_on_the_host(W, H, use_alpha, use_weight, scale_by_alpha):
    lib = _shim()
    im, depth, want = ref_image(W, H, use_alpha, use_weight, scale_by_alpha)
    got = _host_image(lib, im, depth, W, H, use_alpha, use_weight, scale_by_alpha, True)
    hold(got, want, f"host, loss {W}x{H} alpha={use_alpha} weight={use_weight} scale_by_alpha={scale_by_alpha}")
    if use_alpha and H >= 16 and W >= 16:
        hole = im["alpha"] == 0
        assert hole.any() and not got["d_depth"][hole].any() and not got["d_alpha"][hole].any()


@pytest.mark.parametrize("use_alpha", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_depth_to_normal_values_and_gradients_on_the_host(W, H, use_alpha):
    lib = _shim()
    im, depth, want = ref_image(W, H, use_alpha, False, False, loss=False)
    got = _host_image(lib, im, depth, W, H, use_alpha, False, False, False)
    hold(got, want, f"host, depth_to_normal {W}x{H} alpha={use_alpha}")
    border = np.ones((H, W), bool)
    border[1:-1, 1:-1] = False
    assert not got["surf"][:, border].any(), "the one-pixel border is zero"
    if W >= 3 and H >= 3:
        length = np.linalg.norm(got["surf"][:, ~border], axis=0)
        assert ((np.abs(length - 1) <= 1e-5) | (length == 0)).all() and (length > 0).sum() >= length.size // 2, "unit, or exactly zero"


def _surf(lib, z, W, H, tx=ref.TAN_FOVX, ty=ref.TAN_FOVY, alpha=None):
    surf = np.zeros((3, H, W), F32)
    lib.hc_depth_normal(H, W, tx, ty, _p(np.ascontiguousarray(z, F32)), _p(alpha), None, None, 0, _p(surf), None)
    return surf


def test_planes_have_their_analytic_normals():
    lib = _shim()
    W, H = 40, 30
    flat = _surf(lib, np.full((H, W), 2.5), W, H)
    assert np.array_equal(flat[:, 1:-1, 1:-1], np.broadcast_to(np.array([0, 0, -1], F32)[:, None, None], (3, H - 2, W - 2)))
    assert not flat[:, 0].any() and not flat[:, -1].any() and not flat[:, :, 0].any() and not flat[:, :, -1].any()
    # a X + b Y + c Z = d sampled in perspective: Z = d / (a rx + b ry + c) along the ray (rx, ry, 1)
    xs = (2 * (np.arange(W) + 0.5) / W - 1) * ref.TAN_FOVX
    ys = (2 * (np.arange(H) + 0.5) / H - 1) * ref.TAN_FOVY
    for a, b, c, d in ((0.3, -0.2, 1.0, 4.0), (-0.5, 0.4, 0.8, 3.0), (0.0, 0.9, 1.0, 5.0)):
        z = d / (a * xs[None, :] + b * ys[:, None] + c)
        assert (z > 0).all()
        want = -np.array([a, b, c]) / np.linalg.norm([a, b, c])   # facing the camera: n . ray < 0
        got = _surf(lib, z, W, H)[:, 1:-1, 1:-1]
        assert np.abs(got - want[:, None, None]).max() <= 1e-5, (a, b, c, d)   # z is rounded to fp32: 6e-8 z / (2 z / W)


def test_zero_depth_regions_give_exact_zeros():
    lib = _shim()
    W, H = 24, 20
    z = np.full((H, W), 3.0, F32)
    z[5:15, 6:18] = 0.0
    surf = _surf(lib, z, W, H)
    assert np.isfinite(surf).all() and not surf[:, 7:13, 8:16].any(), "inside the hole every neighbour is zero: n = 0 exactly"
    alpha = np.full((H, W), 0.7, F32)
    alpha[5:15, 6:18] = 0.0
    d = (np.full((H, W), 3.0, F32) * alpha).astype(F32)
    d[5:15, 6:18] = 123.0   # depth where alpha is zero is not divided: z = 0
    surf2 = _surf(lib, d, W, H, alpha=alpha)
    assert np.isfinite(surf2).all() and not surf2[:, 7:13, 8:16].any()
    got = np.zeros((H, W), F32), np.zeros((H, W), F32)
    lib.hc_depth_normal_bwd(H, W, ref.TAN_FOVX, ref.TAN_FOVY, _p(d), _p(alpha), None, None, 0, 0.0, _p(np.ones((3, H, W), F32)),
                            _p(got[0]), _p(got[1]), None)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and not got[0][alpha == 0].any() and not got[1][alpha == 0].any()


def test_pixel_centres_are_those_of_ndc2pix():
    """The ray through pixel x has the NDC coordinate that ndc2pix maps back to x: the convention every forward uses."""
    lib = _shim()
    for W, H in ((16, 16), (37, 29), (1600, 1062)):
        for x, y in ((0, 0), (W - 1, H - 1), (W // 3, H // 2)):
            r = np.zeros(2, np.float64)
            lib.hc_ray(W, H, ref.TAN_FOVX, ref.TAN_FOVY, x, y, _p(r))
            assert r[0] == pytest.approx((2 * (x + 0.5) / W - 1) * float(F32(ref.TAN_FOVX)), rel=1e-12, abs=1e-15)
            assert r[1] == pytest.approx((2 * (y + 0.5) / H - 1) * float(F32(ref.TAN_FOVY)), rel=1e-12, abs=1e-15)
            assert lib.hc_ndc2pix(F32(r[0] / float(F32(ref.TAN_FOVX))), W) == pytest.approx(x, abs=2e-4 * W / 1600 + 1e-5)
            assert lib.hc_ndc2pix(F32(r[1] / float(F32(ref.TAN_FOVY))), H) == pytest.approx(y, abs=2e-4 * H / 1062 + 1e-5)


@pytest.mark.parametrize("name,extra", [("hostcheck_normals", ()),
                                        ("hostcheck_normals_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                                   "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_stand_alone_program_plain_and_sanitised(name, extra):
    """The shim's own main sweeps every function over its edge inputs (zero and huge quaternions, ties, 1-pixel images, alpha on
    both sides of its constant); the second build runs it under ASan / UBSan: a stand-alone program, never loaded into Python."""
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    exe = os.path.join(HERE, "hostcheck_normals", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [SRC] + hb._headers()):
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", *hb.EXACT, "-DHOSTCHECK_NORMALS_MAIN", *extra,
                               "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("checksum ") and out.stdout.strip().endswith("bad 0")


# ---- the ABI and the Python surface --------------------------------------------------------------------------------------------

NAMES = {"r3dgs_gaussian_normals", "r3dgs_gaussian_normals_backward", "r3dgs_depth_normal_workspace_bytes", "r3dgs_depth_normal",
         "r3dgs_depth_normal_backward"}


def test_abi_rows_match_the_header():
    from diff_gaussian_rasterization import _C
    from tests import test_abi_table as abi
    protos, rows = abi.header_prototypes(), _C._ABI["required"][1]
    assert NAMES <= set(protos) and NAMES <= set(rows)
    for name in NAMES:
        ret, kinds = protos[name]
        assert abi.ctypes_kind(rows[name][0]) == ret and [abi.ctypes_kind(t) for t in rows[name][1]] == kinds, name
    lib = _C._lib
    assert lib.r3dgs_depth_normal_workspace_bytes(0, 3) == 0 and lib.r3dgs_depth_normal_workspace_bytes(3, -1) == 0
    assert lib.r3dgs_depth_normal_workspace_bytes(8, 32) == 8 and lib.r3dgs_depth_normal_workspace_bytes(9, 33) == 32
    import r3dgs_normals
    header = open(os.path.join(os.path.dirname(HERE), "include", "r3dgs_normals.h")).read()
    assert f"#define R3DGS_NORMAL_ALPHA_MIN {r3dgs_normals.ALPHA_MIN:g}f".replace("0.001", "1e-3") in header
    assert "#define R3DGS_NORMAL_CROSS_MIN 1e-24f" in header and r3dgs_normals.CROSS_MIN == 1e-24 == ref.CROSS_MIN
    assert r3dgs_normals.ALPHA_MIN == ref.ALPHA_MIN


def test_library_refuses_what_the_header_says():
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    err = lambda: lib.r3dgs_last_error().decode()
    n = None
    assert lib.r3dgs_gaussian_normals(0, n, n, n, 0, n, n, n, n) == 0, "P == 0 is valid"
    assert lib.r3dgs_gaussian_normals(10, n, n, n, 0, n, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_gaussian_normals_backward(0, n, n, n, 0, n, n, n, n, n) == 0
    assert lib.r3dgs_gaussian_normals_backward(10, n, n, n, 1, n, n, n, n, n) < 0 and "is NULL" in err()
    assert lib.r3dgs_depth_normal(0, 5, 1.0, 1.0, n, n, n, n, 1, n, n, n, n) == 0
    assert lib.r3dgs_depth_normal(4, 5, 1.0, 1.0, n, n, n, n, 1, n, n, n, n) < 0 and "depth is NULL" in err()
    assert lib.r3dgs_depth_normal(4, 5, 0.0, 1.0, n, n, n, n, 1, n, n, n, n) < 0 and "must be positive" in err()
    assert lib.r3dgs_depth_normal(1 << 16, 1 << 16, 1.0, 1.0, n, n, n, n, 1, n, n, n, n) < 0 and "exceeds" in err()
    assert lib.r3dgs_depth_normal_backward(0, 5, 1.0, 1.0, n, n, n, n, 1, n, n, n, n, n, n) == 0
    assert lib.r3dgs_depth_normal_backward(4, 5, 1.0, 1.0, n, n, n, n, 1, n, n, n, n, n, n) < 0 and "depth is NULL" in err()


def test_python_refusals_before_any_launch():
    import r3dgs_normals as rn
    rs = types.SimpleNamespace(viewmatrix=torch.eye(4), campos=torch.zeros(3), tanfovx=0.5, tanfovy=0.5)
    m, s, q = torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4, 4)
    with pytest.raises(ValueError, match="gaussian_normals: means3D is a host tensor.*no CPU path"):
        rn.gaussian_normals(m, s, q, rs)
    with pytest.raises(ValueError, match="gaussian_normals: means3D is torch.float64"):
        rn.gaussian_normals(m.double(), s, q, rs)
    with pytest.raises(ValueError, match=r"gaussian_normals: means3D has shape \(4, 2\)"):
        rn.gaussian_normals(torch.zeros(4, 2), s, q, rs)
    with pytest.raises(ValueError, match="gaussian_normals: means3D must be a tensor"):
        rn.gaussian_normals(None, s, q, rs)
    for sc, rot in ((None, q), (s, None), (None, None)):
        with pytest.raises(ValueError, match="cov3D_precomp.*no axis to pick"):
            rn.gaussian_normals(m, sc, rot, rs)
    d = torch.zeros(1, 4, 5)
    with pytest.raises(ValueError, match="depth_to_normal: depth is a host tensor"):
        rn.depth_to_normal(d, rs)
    with pytest.raises(ValueError, match=r"depth_to_normal: depth must be a \[1,H,W\] tensor, got \(4, 5\)"):
        rn.depth_to_normal(d[0], rs)
    with pytest.raises(ValueError, match="normal_consistency: depth is torch.float16"):
        rn.normal_consistency(torch.zeros(3, 4, 5), d.half(), rs)
    with pytest.raises(ValueError, match="normal_consistency: normal_map is None"):
        rn.normal_consistency(None, d, rs)
    if torch.cuda.is_available():   # shapes and devices of the other tensors are checked against depth's
        dd = d.cuda()
        with pytest.raises(ValueError, match=r"normal_consistency: normal_map has shape \(3, 4, 4\)"):
            rn.normal_consistency(torch.zeros(3, 4, 4).cuda(), dd, rs)
        with pytest.raises(ValueError, match="normal_consistency: alpha is a host tensor"):
            rn.normal_consistency(torch.zeros(3, 4, 5).cuda(), dd, rs, alpha=d)
        with pytest.raises(ValueError, match=r"normal_consistency: pixel_weight has shape \(1, 4, 5\)"):
            rn.normal_consistency(torch.zeros(3, 4, 5).cuda(), dd, rs, pixel_weight=dd)
        with pytest.raises(ValueError, match="gaussian_normals: scales is a host tensor"):
            rn.gaussian_normals(m.cuda(), s, q.cuda(), rs)


# ---- render(): the keyword, its refusals, and the path with the keyword off --------------------------------------------------------

class _Pipe:
    debug = compute_cov3D_python = convert_SHs_python = False


def _fake_model(P=4):
    pc = types.SimpleNamespace(_xyz=torch.zeros(P, 3), _features_dc=torch.zeros(P, 1, 3), _features_rest=torch.zeros(P, 15, 3),
                               _opacity=torch.zeros(P, 1), _scaling=torch.zeros(P, 3), _rotation=torch.zeros(P, 4),
                               _degrees=torch.zeros(P, 1, dtype=torch.int32), active_sh_degree=3, max_sh_degree=3)
    pc.get_xyz = pc._xyz
    return pc


def _fake_camera(grad=False):
    return types.SimpleNamespace(image_height=8, image_width=8, FoVx=1.0, FoVy=1.0, world_view_transform=torch.eye(4, requires_grad=grad),
                                 full_proj_transform=torch.eye(4), camera_center=torch.zeros(3))


def test_normals_off_is_todays_call_and_touches_no_new_entry_point(monkeypatch):
    import r3dgs_normals
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    calls, touched = [], []
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: calls.append((a, k)) or {"render": None})
    for name in ("gaussian_normals", "depth_to_normal", "normal_consistency"):
        monkeypatch.setattr(r3dgs_normals, name, lambda *a, _n=name, **k: touched.append(_n))
    monkeypatch.setattr(r3dgs_normals, "_lib", types.SimpleNamespace())   # any r3dgs_* call would raise AttributeError
    monkeypatch.setattr(_C, "forward_state", lambda: touched.append("recorder"))
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    r3dgs_render.render(cam, pc, _Pipe, bg)
    r3dgs_render.render(cam, pc, _Pipe, bg, normals=False, scaling_modifier=0.5)
    assert calls == [((cam, pc, _Pipe, bg), {}), ((cam, pc, _Pipe, bg), {"scaling_modifier": 0.5})] and not touched


def test_normals_keyword_rides_the_feature_launch(monkeypatch):
    import contextlib

    import r3dgs_normals
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    seen = []
    n = torch.arange(12.0).reshape(4, 3)

    def fake_normals(means3D, scales, rotations, rs, raw=False):
        seen.append(("normals", means3D, scales, rotations, raw, rs.image_width))
        return n

    def fake_map(features, camera, out, state, rs, inputs=None):
        seen.append(("blend", features))
        return torch.stack([torch.full((8, 8), float(c)) for c in range(features.shape[1])])

    @contextlib.contextmanager
    def recorder():
        yield types.SimpleNamespace(result=None)
    monkeypatch.setattr(r3dgs_normals, "gaussian_normals", fake_normals)
    monkeypatch.setattr(r3dgs_render, "_feature_map", fake_map)
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: {"render": torch.zeros(3, 8, 8)})
    monkeypatch.setattr(_C, "forward_state", recorder)
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    out = r3dgs_render.render(cam, pc, _Pipe, bg, normals=True)
    assert set(out) == {"render", "normal"} and out["normal"].shape == (3, 8, 8)
    kind, means3D, scales, rotations, raw, width = seen[0]
    assert kind == "normals" and raw is True and rotations is pc._rotation and width == 8, "the raw tensors on the fused route"
    assert torch.equal(means3D, pc._xyz) and torch.equal(scales, pc._scaling) and seen[1][1] is n
    # with the user's features: one launch, the normals behind the user's channels
    seen.clear()
    monkeypatch.setattr(r3dgs_render, "_checked_features", lambda *a: None)   # (refuses host tensors, all this test has)
    F = torch.ones(4, 5)
    out = r3dgs_render.render(cam, pc, _Pipe, bg, normals=True, features=F)
    assert [s[0] for s in seen] == ["normals", "blend"] and torch.equal(seen[1][1], torch.cat((F, n), 1))
    assert out["features"].shape == (5, 8, 8) and out["normal"].shape == (3, 8, 8)
    assert out["normal"][:, 0, 0].tolist() == [5.0, 6.0, 7.0] and out["features"][:, 0, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    # a model render() does not rasterize from raw parameters: the activated tensors, raw=False
    seen.clear()
    pc2 = _fake_model()
    pc2._rotation = pc2._rotation.t().contiguous().t()   # not contiguous: not the fused route
    pc2.get_scaling, pc2.get_rotation = torch.ones(4, 3), torch.ones(4, 4)
    r3dgs_render.render(cam, pc2, _Pipe, bg, normals=True)
    assert seen[0][4] is False and seen[0][3] is pc2.get_rotation


def test_render_refusals(monkeypatch):
    import r3dgs_normals
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    from r3dgs_quantised import QuantisedModel
    launched = []
    monkeypatch.setattr(r3dgs_render, "_render", lambda *a, **k: launched.append("render"))
    monkeypatch.setattr(r3dgs_render, "_render_quantised", lambda *a, **k: launched.append("quantised"))
    monkeypatch.setattr(r3dgs_normals, "gaussian_normals", lambda *a, **k: launched.append("normals"))
    cam, pc, bg = _fake_camera(), _fake_model(), torch.zeros(3)
    qm = object.__new__(QuantisedModel)
    with pytest.raises(ValueError, match="normals=True is not available for a QuantisedModel"):
        r3dgs_render.render(cam, qm, _Pipe, bg, normals=True)

    class CovPipe(_Pipe):
        compute_cov3D_python = True
    with pytest.raises(ValueError, match="normals=True together with pipe.compute_cov3D_python"):
        r3dgs_render.render(cam, pc, CovPipe, bg, normals=True)
    with pytest.raises(ValueError, match="normals=True together with a camera that requires grad"):
        r3dgs_render.render(_fake_camera(grad=True), pc, _Pipe, bg, normals=True)
    with pytest.raises(ValueError, match=r"C \+ 3 <= 512 channels, got C = 510"):
        r3dgs_render.render(cam, pc, _Pipe, bg, normals=True, features=torch.zeros(4, _C.FEATURE_MAX_CHANNELS - 2))
    with pytest.raises(ValueError, match="features_geom_grad=True under no_grad"), torch.no_grad():
        r3dgs_render.render(cam, pc, _Pipe, bg, normals=True, features_geom_grad=True)
    with pytest.raises(ValueError, match="features_geom_grad=True without features"):
        r3dgs_render.render(cam, pc, _Pipe, bg, features_geom_grad=True)
    assert not launched, "a refused call launched something"
