"""CPU checks of the auxiliary maps (include/r3dgs_aux.h, reduced-3dgs_amd/csrc/aux_math.h, csrc/aux_maps.hip): the numpy
restatement tests/aux_ref.py pinned by hand cases and against the oracle's own walk; the step function run on the host by the
stand-alone program tests/hostcheck_aux/hostcheck_aux.hip, plainly and under the host sanitizers; the seeded scenes of the
GPU tests held inside the ambiguity caps by the reference alone; and the host surface (ABI row, both bindings, render's
keyword).  No GPU needed."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aux_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
F = np.float32
AMBIG_MAX_FRACTION = 1e-3   # the project's cap on flagged pixels (tests/test_gpu_parity.py)


def centred(x, y, op, z):
    """An isotropic unit conic centred on pixel (x, y): power = 0 there, alpha = min(0.99, op)."""
    return (x, y, 1.0, 0.0, 1.0, op, z)


def at(res, name, x=5, y=9):
    return res[name][y, x]


def test_one_gaussian_over_a_pixel():
    """depth = z alpha; the median is z when alpha > 0.5 and 0 otherwise."""
    for op, want_median in ((0.6, 4.0), (0.3, 0.0), (0.5, 0.0)):
        r = ar.aux_ref(ar.hand_state([centred(5, 9, op, 4.0)]))
        assert at(r, "depth") == F(4.0) * F(op) * F(1.0)
        assert at(r, "alpha") == F(1.0) - (F(1.0) - F(op))
        assert at(r, "median_depth") == F(want_median)
        assert at(r, "last") == 1
    # off the centre the falloff applies: alpha = op * exp(-0.5 * d^2)
    r = ar.aux_ref(ar.hand_state([centred(5, 9, 0.9, 4.0)]))
    a = F(0.9) * np.exp(F(-0.5) * F(4.0))
    assert r["depth"][9, 7] == F(4.0) * a * F(1.0) and r["median_depth"][9, 7] == 0.0


def test_two_gaussians_cross_at_the_second():
    r = ar.aux_ref(ar.hand_state([centred(5, 9, 0.3, 2.0), centred(5, 9, 0.3, 3.0)]))
    T1 = F(1.0) * (F(1.0) - F(0.3))
    assert at(r, "depth") == F(2.0) * F(0.3) * F(1.0) + F(3.0) * F(0.3) * T1
    assert at(r, "final_T") == T1 * (F(1.0) - F(0.3)) and at(r, "final_T") < 0.5 < T1
    assert at(r, "median_depth") == 3.0 and at(r, "last") == 2


def test_saturated_pixel_stops_where_the_forward_stops():
    """T = 0.05, 0.0025, 1.25e-4; the fourth entry would leave 6.25e-6 < 1e-4: it and everything behind it is not blended."""
    st = ar.hand_state([centred(5, 9, 0.95, 1.0 + k) for k in range(6)])
    assert st["n_contrib"].reshape(16, 16)[9, 5] == 3
    r = ar.aux_ref(st)
    assert at(r, "last") == 3 and at(r, "median_depth") == 1.0
    want, T = F(0.0), F(1.0)
    for k in range(3):
        want = want + F(1.0 + k) * F(0.95) * T
        T = T * (F(1.0) - F(0.95))
    assert at(r, "depth") == want and at(r, "final_T") == T


def test_skipped_entries_leave_no_trace():
    """alpha < 1/255 and power > 0 entries count as list positions and as nothing else."""
    plain = ar.aux_ref(ar.hand_state([centred(5, 9, 0.3, 2.0), centred(5, 9, 0.3, 3.0)]))
    faint = ar.aux_ref(ar.hand_state([centred(5, 9, 0.3, 2.0), centred(5, 9, 0.003, 100.0), centred(5, 9, 0.3, 3.0)]))
    indefinite = ar.aux_ref(ar.hand_state([centred(5, 9, 0.3, 2.0), (6, 9, -1.0, 0.0, -1.0, 0.9, 100.0), centred(5, 9, 0.3, 3.0)]))
    for r in (faint, indefinite):
        for name in ("depth", "alpha", "median_depth", "final_T"):
            assert at(r, name) == at(plain, name), name
        assert at(r, "last") == 3
    # (the indefinite conic has power = +0.5 at the pixel: skipped by the first rule, not by the second)


def test_empty_pixel_and_empty_list():
    r = ar.aux_ref(ar.hand_state([centred(5, 9, 0.9, 4.0)]))
    far = (15, 0)   # alpha = 0.9 exp(-0.5 * 181) < 1/255
    for name in ("depth", "alpha", "median_depth"):
        assert r[name][far[1], far[0]] == 0.0
    assert r["last"][far[1], far[0]] == 0
    r = ar.aux_ref(ar.hand_state(np.zeros((0, 7))))
    assert not r["depth"].any() and not r["alpha"].any() and not r["median_depth"].any() and not r["median_ambig"].any()


def test_median_ambiguity_mask():
    """A pixel whose T lands within 1e-4 (relative) of 0.5 after a blended entry is flagged; one further away is not."""
    near = ar.aux_ref(ar.hand_state([centred(5, 9, 0.50002, 4.0)]))
    assert at(near, "median_ambig") and not near["median_ambig"][9, 7]
    clear = ar.aux_ref(ar.hand_state([centred(5, 9, 0.51, 4.0)]))
    assert not at(clear, "median_ambig") and at(clear, "median_depth") == 4.0


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, kw in (("A", ar.SCENE_A), ("B", ar.SCENE_B)):
        cam, g, bg = ar.make_scene(kw)
        ref = orc.forward(bg, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None,
                          cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, kw["H"], kw["W"], g["sh"],
                          g["degrees"], cam.camera_center, want_ambig=True, ambig_rel=1e-5)
        out[name] = (kw, ref, ar.aux_ref(ref["state"]))
    return out


def test_restatement_walks_as_the_oracle_walks(scenes):
    """Over the oracle's lists the restatement blends the entries the oracle blended: the same last contributor on every
    pixel the oracle does not flag, the same final T to an ulp of 1 (numpy's exp against libm's)."""
    for name, (kw, ref, a) in scenes.items():
        st = ref["state"]
        ok = ref["ambig"].reshape(-1) == 0
        np.testing.assert_array_equal(a["last"].reshape(-1)[ok], st["n_contrib"][ok])
        assert np.abs(a["final_T"].reshape(-1) - st["final_T"])[ok].max() <= 2.0 ** -22
        assert (a["depth"] >= 0).all() and a["depth"].max() <= st["depths"][st["radii"] > 0].max()
        crossed = a["median_depth"] > 0
        assert (a["final_T"][~crossed & ~a["median_ambig"]] >= 0.5).all() and (a["final_T"][crossed] < 0.5 + 1e-4).all()


def test_the_gpu_scenes_stay_inside_both_caps(scenes):
    """Measured (reference lists): scene A 0.0000 % oracle-ambiguous, 0.0571 % median-ambiguous; scene B 0 % and 0 %."""
    for name, (kw, ref, a) in scenes.items():
        amb, med = float((ref["ambig"] != 0).mean()), float(a["median_ambig"].mean())
        print(f"[aux scene {name}] oracle-ambiguous {100 * amb:.4f} %, median-ambiguous {100 * med:.4f} %")
        assert amb <= AMBIG_MAX_FRACTION and med <= AMBIG_MAX_FRACTION
    kw, ref, a = scenes["A"]
    assert kw["W"] % 16 and kw["H"] % 16 and kw["P"] == 2000 and (kw["W"], kw["H"]) == (100, 70)
    assert len(set(ar.make_scene(kw)[1]["degrees"].reshape(-1).tolist())) > 1, "mixed degrees"
    assert 0.2 < (a["median_depth"] > 0).mean() < 0.95, "the median map is neither empty nor full"


def _build_hostcheck(name, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "tests", "hostcheck_aux", "hostcheck_aux.hip")
    exe = os.path.join(ROOT, "tests", "hostcheck_aux", name)
    hdrs = [os.path.join(ROOT, "reduced-3dgs_amd", "csrc", h) for h in ("aux_math.h", "blend_math.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-DR3_TRIP_FORMS_ON_HOST", "-ffp-contract=off",
                               *extra, "-o", exe, src])
    return exe


@pytest.mark.parametrize("name,extra", [("hostcheck_aux", ()),
                                        ("hostcheck_aux_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                               "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_step_function_on_the_host(name, extra):
    """aux_math.h's step against a double restatement (bounds stated in the program), plainly and as a second copy with the
    host side under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    out = subprocess.run([_build_hostcheck(name, extra)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1].startswith("hostcheck_aux: OK"), out.stdout[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_build_compiles_the_unit_as_the_forward_blend():
    import build
    assert build.UNITS["aux_maps.hip"] == build.UNITS["blend.hip"]


def test_host_surface():
    import torch

    import diff_gaussian_rasterization as dgr
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    assert "r3dgs_aux_maps" in _C._ABI["required"][1] and hasattr(_C._lib, "r3dgs_aux_maps")
    assert len(_C._ABI["required"][1]["r3dgs_aux_maps"][1]) == 13
    assert ("r3dgs_aux_maps", True) in _C._ext_loaded.entry_points()
    assert len(dgr.GaussianRasterizationSettings._fields) == 12
    # `aux` is a keyword on top of the reference's signature, which inspect.signature keeps reporting (functools.wraps)
    assert "aux" not in inspect.signature(r3dgs_render.render).parameters
    assert r3dgs_render.render.__kwdefaults__ == {"aux": None}
    assert _C.AUX_MAPS == ("depth", "alpha", "median_depth")
    # no CPU path: host buffers are refused with the message of every other entry point, by both bindings
    blobs = [torch.zeros(64, dtype=torch.uint8) for _ in range(3)]
    for binding in ("torch", "ctypes"):
        was = _C.set_binding(binding)
        try:
            with pytest.raises(RuntimeError, match="no CPU path"):
                _C.aux_maps(4, 16, 16, 16, *blobs)
            with pytest.raises(RuntimeError, match="no CPU path"):
                dgr.aux_maps(4, 16, 16, 16, *blobs, maps=("alpha",))
            with pytest.raises(ValueError, match="unknown map"):
                _C.aux_maps(4, 16, 16, 16, *blobs, maps=("depth", "normal"))
        finally:
            _C.set_binding(was)
    with pytest.raises(ValueError, match="unknown aux map"):
        r3dgs_render.render(None, None, None, None, aux=("colour",))
