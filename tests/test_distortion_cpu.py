"""CPU checks of the depth-distortion map (include/r3dgs_distortion.h, csrc/distortion_math.h): the float64 reference
tests/distortion_ref.py pinned by hand states with closed forms, by the identity the backward builds on and by central finite
differences; the scenes of the GPU tests held inside the project's cap on flagged pixels by the reference alone; an fp32 numpy
restatement of the kernel's shifted forward held inside the GPU value bar on each of them (and the unshifted fp32 form shown to
miss it on the FAR scene); the shared forward step, backward step and per-Gaussian chain run on the host by the stand-alone
program tests/hostcheck_distortion/hostcheck_distortion.hip over a seeded scene, plainly and under the host sanitizers, against
that reference; the host surface.  No GPU needed."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import distortion_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels
PIX = 9 * 16 + 5           # pixel (5, 9) of the one-tile hand states
NEAR_FAR = (0.5, 20.0)


def centred(op, z, x=5, y=9):
    """An isotropic unit conic centred on pixel (x, y): G = 1 there, alpha = min(0.99, op)."""
    return (x, y, 1.0, 0.0, 1.0, op, z)


def one_hot(value=1.0):
    g = np.zeros(256)
    g[PIX] = value
    return g


@pytest.mark.parametrize("mapping", [(0.0, 0.0), NEAR_FAR])
def test_one_gaussian_gives_zero(mapping):
    st = ar.hand_state([centred(0.6, 4.0)])
    r = dr.state_grads(st, np.ones(256), *mapping)
    assert not r["map"].any()
    for k in ("xy", "conic_op", "depths"):
        assert not r[k].any(), k


@pytest.mark.parametrize("mapping", [(0.0, 0.0), NEAR_FAR])
def test_two_gaussians_closed_form(mapping):
    """distortion = a0 a1 (1 - a0) (m0 - m1)^2 at the centre, with its derivatives in a0, a1, m0, m1 (dm/dz by the mapping)."""
    a0, a1, z0, z1 = np.float64(np.float32(0.3)), np.float64(np.float32(0.45)), 2.0, 3.5
    near, far = mapping
    st = ar.hand_state([centred(a0, z0), centred(a1, z1)])
    m0, m1 = dr.mapped(z0, near, far), dr.mapped(z1, near, far)
    dmdz = [1.0, 1.0] if near == 0.0 else [far * near / ((far - near) * z * z) for z in (z0, z1)]
    r = dr.state_grads(st, one_hot(), near, far)
    d = m0 - m1
    np.testing.assert_allclose(r["map"][PIX], a0 * a1 * (1 - a0) * d * d, rtol=1e-12)
    np.testing.assert_allclose(r["conic_op"][:, 3], [a1 * (1 - 2 * a0) * d * d, a0 * (1 - a0) * d * d], rtol=1e-10)
    dm0 = 2 * a0 * a1 * (1 - a0) * d
    np.testing.assert_allclose(r["depths"], [dm0 * dmdz[0], -dm0 * dmdz[1]], rtol=1e-10)
    assert not r["xy"].any()   # at the centre the falloff is flat


def test_equal_depths_give_zero():
    st = ar.hand_state([centred(0.3, 2.5), centred(0.5, 2.5), (6, 8, 0.5, 0.1, 0.7, 0.4, 2.5)])
    r = dr.state_grads(st, np.ones(256))
    assert np.abs(r["map"]).max() <= 1e-14   # (the float64 reference's own rounding of z^2 ~ 6: a few 1e-16)
    for k in ("xy", "conic_op", "depths"):
        assert np.abs(r[k]).max() <= 1e-14, k


def seeded_state():
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    ref = orc.forward(np.zeros(3, np.float32), g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None,
                      cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, kw["H"], kw["W"], g["sh"],
                      g["degrees"], cam.camera_center)
    return ref["state"]


@pytest.mark.parametrize("mapping", [(0.0, 0.0), NEAR_FAR])
def test_totals_identity(mapping):
    """A S2 - S1^2 equals the prefix form at 1e-10 (relative to the map's maximum), and A = 1 - final_T."""
    import torch
    st = seeded_state()
    with torch.no_grad():
        m = dr.walk(st, dr._t(st["xy"]), dr._t(st["conic_op"]), dr._t(st["depths"]), *mapping)
    a, b = m["distortion"].numpy(), m["totals"].numpy()
    assert a.max() > 1e-3
    assert np.abs(a - b).max() <= 1e-10 * max(1.0, a.max())
    assert (a >= -1e-15).all()


def test_reference_gradients_against_finite_differences():
    st = ar.hand_state([(5.3, 8.6, 0.6, 0.1, 0.5, 0.5, 2.0), (6.1, 9.2, 0.4, -0.05, 0.7, 0.6, 2.8), (4.2, 9.9, 0.5, 0.0, 0.5, 0.7, 3.1)])
    rng = np.random.default_rng(3)
    g = rng.uniform(-1, 1, 256)
    for mapping in ((0.0, 0.0), NEAR_FAR):
        r = dr.state_grads(st, g, *mapping)

        def loss(key, idx, h):
            s = dict(st)
            arr = np.asarray(st[key], np.float64).copy()
            arr[idx] += h
            s[key] = arr
            # the decisions stay the state's own fp32 ones: only the float64 values move
            import torch
            with torch.no_grad():
                m = dr.walk(st, *[dr._t(s[k]) for k in ("xy", "conic_op", "depths")], *mapping)["distortion"].numpy()
            return float((g * m).sum())
        for key, idx in (("xy", (0, 0)), ("xy", (1, 1)), ("conic_op", (0, 0)), ("conic_op", (1, 1)), ("conic_op", (2, 2)),
                         ("conic_op", (1, 3)), ("depths", (0,)), ("depths", (2,))):
            h = 1e-6
            fd = (loss(key, idx, h) - loss(key, idx, -h)) / (2 * h)
            np.testing.assert_allclose(r[key][idx], fd, rtol=1e-6, atol=1e-9)


@pytest.fixture(scope="module")
def scene_states():
    out = {}
    for name, cam, g, H, W, mappings in dr.gpu_scenes():
        ref = orc.forward(np.array([0.1, 0.3, 0.2], np.float32), g["means3D"], None, g["opacity"], g["scales"], g["rotations"],
                          1.0, None, cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"],
                          g["degrees"], cam.camera_center, want_ambig=True)
        out[name] = (ref, mappings)
    return out


def test_gpu_scenes_stay_inside_the_flag_cap(scene_states):
    for name, (ref, _) in scene_states.items():
        share = (ref["ambig"] != 0).mean()
        print(f"[distortion {name}] oracle-ambiguous {100 * share:.4f} % (cap {100 * FLAG_MAX_FRACTION:.2f} %)")
        assert share <= FLAG_MAX_FRACTION, name


def test_far_scene_is_far(scene_states):
    st = scene_states["FAR"][0]["state"]
    z = st["depths"][st["radii"] > 0]
    assert 99.5 <= z.min() and z.max() <= 104.5 and z.max() - z.min() > 3.0
    assert np.asarray(st["n_contrib"]).max() >= 8


def test_fp32_restatement_meets_the_gpu_value_bar(scene_states):
    """The kernel's arithmetic restated in numpy -- fp32 weights, fp32 shifted mapped depths, double running sums -- stays
    inside |got - ref| <= 1e-5 max(1, max |ref|) on every GPU test scene; with fp32 running sums the figure is printed.  On FAR
    the UNSHIFTED fp32 form (raw z ~ 100) misses the bar: the shift is what makes it reachable."""
    for name, (ref, mappings) in scene_states.items():
        st = ref["state"]
        for near, far in mappings:
            want = dr.reference_map(st, near, far)
            bar = 1e-5 * max(1.0, np.abs(want).max())
            err = np.abs(dr.shifted_fp32(st, near, far)["distortion"].astype(np.float64) - want).max()
            err32 = np.abs(dr.shifted_fp32(st, near, far, acc=np.float32)["distortion"].astype(np.float64) - want).max()
            print(f"[distortion {name} ({near}, {far})] max |ref| {np.abs(want).max():.3e}, restatement error {err:.3e} "
                  f"(fp32 sums: {err32:.3e}), bar {bar:.3e}")
            assert np.abs(want).max() > 0
            assert err <= bar, (name, near, far, err, bar)
    st = scene_states["FAR"][0]["state"]
    want = dr.reference_map(st)
    # raw moments: the exact totals over the unshifted depths, merely STORED in fp32, already lose A S2 - S1^2
    import torch
    with torch.no_grad():
        m = dr.walk(st, dr._t(st["xy"]), dr._t(st["conic_op"]), dr._t(st["depths"]))
    a, s1, s2 = (m[k].numpy().astype(np.float32) for k in ("A", "S1", "S2"))
    unshifted = (a * s2 - s1 * s1).astype(np.float64)
    assert np.abs(unshifted - want).max() > 1e-5 * max(1.0, np.abs(want).max()), "FAR must defeat raw fp32 moments"


REL = 1e-4                      # the project's gradient bar: max err <= 1e-4 * max |ref| per tensor
EPS32 = float(np.finfo(np.float32).eps)
SAN = ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined")


def _build_hostcheck(name, extra):
    """The stand-alone program, by the rule of tests/hostcheck_build.py: rebuilt when its source or any header is newer."""
    import subprocess
    from tests import hostcheck_build as hb
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "tests", "hostcheck_distortion", "hostcheck_distortion.hip")
    exe = os.path.join(ROOT, "tests", "hostcheck_distortion", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hb._headers()):
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def host_scene(tmp_path_factory):
    """SCENE_17 (P = 300, 17x17: two tiles a side, one pixel wide at the edge), its oracle state, a seeded upstream gradient (zero
    on flagged pixels), the reference under both mappings and the scene files of the host program: the linear mapping with the
    chain in double, 2DGS's with the chain in fp32."""
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    H, W, P = kw["H"], kw["W"], kw["P"]
    ref = orc.forward(np.array([0.1, 0.3, 0.2], np.float32), g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0,
                      None, cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"],
                      g["degrees"], cam.camera_center, want_ambig=True)
    st = ref["state"]
    ok = ref["ambig"].reshape(-1) == 0
    up = np.random.default_rng(7).uniform(-1.0, 1.0, H * W).astype(np.float32) * ok
    ranges, plist = np.asarray(st["ranges"]).reshape(-1, 2), np.asarray(st["point_list"]).reshape(-1)
    R = int(ranges[:, 1].max()) if len(ranges) else 0
    d = tmp_path_factory.mktemp("distortion")
    cases = {}
    for (near, far), f64 in (((0.0, 0.0), True), (NEAR_FAR, False)):
        path = str(d / f"scene_{int(f64)}.txt")
        with open(path, "w") as f:
            f.write(f"{W} {H} {P} {R} {len(ranges)} {int(f64)} {cam.tanfovx!r} {cam.tanfovy!r} 1.0 {near!r} {far!r}\n")
            for m in (cam.world_view_transform, cam.full_proj_transform):
                f.write(" ".join(repr(float(v)) for v in np.asarray(m, np.float32).reshape(-1)) + "\n")
            f.write(" ".join(str(int(v)) for v in ranges.reshape(-1)) + "\n")
            f.write(" ".join(str(int(v)) for v in plist[:R]) + "\n")
            for k in range(H * W):
                f.write(f"{int(st['n_contrib'][k])} {float(st['final_T'][k])!r} {float(up[k])!r}\n")
            for i in range(P):
                row = [int(st["radii"][i])] + [float(v) for v in st["xy"][i]] + [float(v) for v in st["conic_op"][i]] + \
                      [float(st["depths"][i])] + [float(v) for v in g["means3D"][i]] + [float(v) for v in g["scales"][i]] + \
                      [float(v) for v in g["rotations"][i]]
                f.write(" ".join(repr(v) for v in row) + "\n")
        want = dr.reference_grads(st, g["means3D"], g["opacity"], g["scales"], g["rotations"], cam.world_view_transform,
                                  cam.full_proj_transform, cam.tanfovx, cam.tanfovy, up, near, far)
        cases[(near, far)] = dict(path=path, f64=f64, want=want, bound=_forward_bound(st, near, far), ok=ok)
    return dict(P=P, N=H * W, cases=cases)


def _forward_bound(st, near, far):
    """Per-pixel rounding bound of the fp32 forward step against the float64 reference over the same fp32 state.

    The two differ in alpha_k (fp32 power and exp against float64) and in the fp32 products behind it; the sums are double.
      * alpha: log2 G = qa dxx + qb dxy + qc dyy has an absolute error of at most 4 eps mag, mag = |qa dxx| + |qb dxy| + |qc dyy|
        (taken from the state, the largest over the pixel's blended entries), so exp2 moves by at most 4 ln2 mag eps, plus one ulp
        of exp2f and half an ulp of the product with the opacity:  eps_a = (4 ln2 mag + 2) eps  (48 eps at mag = 16).
      * a factor (1 - alpha) of T moves by eps_a alpha / (1 - alpha) <= eps_a amp, amp = max(1, max_k alpha_k / (1 - alpha_k)) over
        the pixel's blended entries; w_k has at most k such factors, alpha_k itself and a rounding each: (n + 2)(eps_a amp + eps).
      * the shifted mapped depth: z - z_ref is exact or one rounding, the 2DGS form three more: 4 eps on m, 8 eps on m^2.
      * distortion = sum_{j<k} w_j w_k (m_k - m_j)^2 is written as a difference of terms of magnitude A S2s (S2s = sum w (m -
        m_ref)^2 >= distortion / A), two weights and one squared depth per term:
          bound = (n + 2) (8 eps + 2 eps_a amp) A S2s  +  half an ulp of the fp32 result."""
    import torch
    W, H = int(st["W"]), int(st["H"])
    with torch.no_grad():
        m = dr.walk(st, dr._t(st["xy"]), dr._t(st["conic_op"]), dr._t(st["depths"]), near, far)
    A, S1, S2, dist = (m[k].numpy() for k in ("A", "S1", "S2", "distortion"))
    mref, amp, magmax = np.zeros(H * W), np.ones(H * W), np.zeros(H * W)
    xy, co = np.asarray(st["xy"], np.float64), np.asarray(st["conic_op"], np.float64)
    z = np.asarray(st["depths"], np.float64)
    for pix, xs, ys, g_first, entries in dr._decisions(st):
        if g_first is not None:
            mref[pix] = dr.mapped(z[g_first], near, far)
        for g, take, alpha32 in entries:
            a = alpha32.astype(np.float64)
            amp[pix] = np.where(take, np.maximum(amp[pix], a / (1.0 - a)), amp[pix])
            dx, dy = xy[g, 0] - xs, xy[g, 1] - ys
            mag = (0.5 * np.abs(co[g, 0]) * dx * dx + 0.5 * np.abs(co[g, 2]) * dy * dy + np.abs(co[g, 1] * dx * dy)) / np.log(2.0)
            magmax[pix] = np.where(take, np.maximum(magmax[pix], mag), magmax[pix])
    S2s = S2 - 2.0 * mref * S1 + mref * mref * A
    n = np.asarray(st["n_contrib"]).reshape(-1).astype(np.float64)
    eps_a = (4.0 * np.log(2.0) * magmax + 2.0) * EPS32
    return (n + 2.0) * (8.0 * EPS32 + 2.0 * eps_a * amp) * A * np.maximum(S2s, 0.0) + 0.5 * EPS32 * np.abs(dist)


@pytest.mark.parametrize("name,extra", [("hostcheck_distortion", ()), ("hostcheck_distortion_san", SAN)])
def test_steps_and_chain_on_the_host(host_scene, name, extra):
    """distortion_math.h's forward and backward steps and aux_math.h's chain on the CPU, in the device passes' order of
    summation: the map within the derived rounding bound of `_forward_bound` on every unflagged pixel, the gradients at the
    project's bar; the second build runs the host side under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
    program, never loaded into Python."""
    import subprocess
    exe = _build_hostcheck(name, extra)
    for (near, far), c in host_scene["cases"].items():
        out = subprocess.run([exe, c["path"]], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        assert lines[-1].startswith("hostcheck_distortion: OK")
        N, P = host_scene["N"], host_scene["P"]
        assert len(lines) == N + P + 1
        pix = np.array([[float(v) for v in ln.split()[2:]] for ln in lines[:N]])
        want = c["want"]
        err = np.abs(pix[:, 0] - want["map"])
        worst = (err / np.maximum(c["bound"], 1e-300))[c["ok"] & (c["bound"] > 0)].max()
        print(f"[hostcheck_distortion ({near}, {far})] forward: max err {err[c['ok']].max():.3e}, max |ref| "
              f"{np.abs(want['map']).max():.3e}, worst err / bound {worst:.3f}")
        assert np.abs(want["map"]).max() > 0
        assert (err <= c["bound"])[c["ok"]].all(), (near, far, worst)
        assert not pix[c["bound"] == 0, 0][c["ok"][c["bound"] == 0]].any()   # nothing or one entry blended: exactly 0
        got = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[N:-1]])
        assert got.shape == (P, 14)
        cols = dict(means2D=got[:, 0:2], means3D=got[:, 2:5], opacity=got[:, 5:6], scales=got[:, 6:9], rotations=got[:, 9:13],
                    z=got[:, 13])
        for k, a in cols.items():
            b = np.asarray(want[k]).reshape(a.shape)
            scale, e = np.abs(b).max(), np.abs(a - b).max()
            print(f"[hostcheck_distortion ({near}, {far}) f64={c['f64']}] {k}: max err {e:.3e}, bar {REL * scale:.3e}")
            assert scale > 0 and e <= REL * scale, (k, near, far, e, scale)


def test_host_surface():
    """The C header declares the three entry points; _C's table has their rows in the required group."""
    hdr = open(os.path.join(ROOT, "include", "r3dgs_distortion.h")).read()
    for name in ("r3dgs_distortion_map(", "r3dgs_distortion_map_backward_workspace_bytes(", "r3dgs_distortion_map_backward("):
        assert name in hdr, name
    src = open(os.path.join(ROOT, "reduced-3dgs_amd", "diff_gaussian_rasterization", "_C.py")).read()
    required = src[src.index('"required": (None, {'):src.index('"params": (')]
    for name in ("r3dgs_distortion_map", "r3dgs_distortion_map_backward_workspace_bytes", "r3dgs_distortion_map_backward"):
        assert f'"{name}":' in required, name
    units = open(os.path.join(ROOT, "reduced-3dgs_amd", "build.py")).read()
    assert '"distortion.hip": ["-ffp-contract=fast"' in units
