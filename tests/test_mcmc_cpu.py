"""CPU checks of the 3DGS-MCMC strategy (reduced-3dgs_amd/r3dgs_mcmc.py, csrc/mcmc.hip, csrc/mcmc_math.h, include/r3dgs_mcmc.h):
the float64 restatement (tests/mcmc_ref.py) is pinned by hand-worked cases; the per-Gaussian kernel arithmetic runs on the host
through a test shim and is held to the restatement -- the relocation formula within the bound derived there, the gate and the
noise term at the GPU tests' bars, the draw search and the ratio clamp exactly; the same shim runs as a stand-alone program,
plain and under ASan/UBSan; the ABI rows, every refusal and the arithmetic of the growth step.  No GPU needed."""
import ctypes as C
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import densify_ref
from tests import hostcheck_build as hb
from tests import mcmc_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_mcmc", "hostcheck_mcmc.hip")
SO = os.path.join(HERE, "hostcheck_mcmc", "libhostcheck_mcmc.so")
F32 = np.float32


def _shim():
    lib = hb.build_shim(SRC, SO, hb.EXACT, "hipcc not available to build the MCMC host-check shim")
    lib.hc_mcmc_binom.restype = C.c_double
    lib.hc_mcmc_binom.argtypes = [C.c_int, C.c_int]
    lib.hc_mcmc_gate.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.hc_mcmc_noise.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_float]
    lib.hc_mcmc_weights.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 4
    lib.hc_mcmc_draw.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.hc_mcmc_relocate_f64.argtypes = [C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.hc_mcmc_relocate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the restatement, pinned by hand ---------------------------------------------------------------------------------------

def test_reference_is_pinned_by_hand_worked_cases():
    for o in (0.01, 0.3, 0.9):
        o2 = ref.relocate_o(o, 2)
        assert ref.relocate_D(o2, 2) == pytest.approx(o2 + o2 - o2 ** 2 / math.sqrt(2), rel=1e-15)
        o3 = ref.relocate_o(o, 3)
        want = o3 + (o3 - o3 ** 2 / math.sqrt(2)) + (o3 - 2 * o3 ** 2 / math.sqrt(2) + o3 ** 3 / math.sqrt(3))
        assert ref.relocate_D(o3, 3) == pytest.approx(want, rel=1e-15)
        for N in (2, 3, 17, 51):
            assert 1 - (1 - ref.relocate_o(o, N)) ** N == pytest.approx(o, rel=1e-13)
            # the row function's log1p / expm1 form is the same number
            L_op, _, _, _ = ref.relocate_row(F32(math.log(o / (1 - o))), np.zeros(3, F32), N, 0.0)
            o_back = 1 / (1 + math.exp(-L_op))
            assert 1 - (1 - o_back) ** N == pytest.approx(float(ref.sigmoid64(F32(math.log(o / (1 - o))))), rel=1e-12)
    assert ref.gate(0.005) == 0.5, "the gate at o = 0.005 is exactly 1/2"
    assert ref.gate(1.0) < 1e-40 and ref.gate(0.0) == pytest.approx(1 / (1 + math.exp(-0.5)))
    assert ref.BINOM[50, 25] == 126410606437752.0 and ref.BINOM[4, 2] == 6 and ref.BINOM[3, 4] == 0
    # a unit quaternion about z by 90 degrees, scales (1, 2, 3): S = diag(4, 1, 9)
    S = ref.covariance(np.array([[math.sqrt(0.5), 0, 0, math.sqrt(0.5)]]), np.log(np.array([[1.0, 2.0, 3.0]])))[0]
    assert np.allclose(S, np.diag([4.0, 1.0, 9.0]), atol=1e-12)
    # draws: weights (0, 1, 0, 3, 0): u = 0 -> 1, u just below 1/4 -> 1, u = 1/4 -> 3, u -> 1: 3; never a zero-weight row
    w = np.array([0.0, 1.0, 0.0, 3.0, 0.0])
    assert ref.draws(w, [0.0, 0.2499999, 0.25, 0.99999994]).tolist() == [1, 1, 3, 3]
    assert ref.ratio_of(4, [1] * 60 + [2])[0].tolist() == [1, 51, 2, 1]


@pytest.mark.parametrize("P,cap,want", [(0, 100, 0), (1, 100, 0), (60, 1000, 3), (1000, 1000, 0), (1000, 900, 0), (1000, 1020, 20),
                                        (1000, 5000, 50), (2857, 3000, 142), (2999, 3000, 1), (19, 1000, 0), (20, 1000, 1)])
def test_the_arithmetic_of_the_growth_step(P, cap, want):
    import r3dgs_mcmc as mc
    assert mc.n_new_rows(P, cap) == ref.n_new(P, cap) == want == max(0, min(cap, int(1.05 * P)) - P)


# ---- mcmc_math.h on the host -------------------------------------------------------------------------------------------------

def test_binomials_are_exact():
    lib = _shim()
    for n in range(51):
        for k in range(51):
            assert lib.hc_mcmc_binom(n, k) == float(math.comb(n, k)), (n, k)


def test_relocation_formula_within_the_derived_bound():
    lib = _shim()
    rng = np.random.default_rng(3)
    n = 4000
    opacity = np.minimum(rng.normal(-1, 2.5, n), math.log(0.99 / 0.01) - 1e-3).astype(F32)
    assert (ref.sigmoid64(opacity) <= 0.99).all()
    scaling = rng.uniform(-8, 1, (n, 3)).astype(F32)
    ratio = rng.integers(2, 52, n).astype(np.int32)
    ratio[:200] = 2
    ratio[200:300] = 51
    got_op, got_sc = np.zeros(n, F32), np.zeros((n, 3), F32)
    lib.hc_mcmc_relocate(n, _p(opacity), _p(scaling), _p(ratio), 0.005, _p(got_op), _p(got_sc))
    worst = [0.0, 0.0]
    largest = 0.0
    for i in range(n):
        L_op, L_sc, b_op, b_sc = ref.relocate_row(opacity[i], scaling[i], int(ratio[i]), 0.005)
        worst[0] = max(worst[0], abs(got_op[i] - L_op) / b_op)
        worst[1] = max(worst[1], float((np.abs(got_sc[i] - L_sc) / b_sc).max()))
        largest = max(largest, b_op, float(b_sc.max()))
    print(f"relocation on the host: worst error / bound: opacity {worst[0]:.3f}, scaling {worst[1]:.3f}; largest bound {largest:.3g}")
    assert worst[0] <= 1 and worst[1] <= 1
    assert largest < 2e-4, "with sigmoid <= 0.99 the bound stays small"
    # o' and D themselves, in double
    for o, N in ((0.5, 2), (0.99, 51), (1e-6, 7), (0.3, 30)):
        o_new, D = C.c_double(), C.c_double()
        lib.hc_mcmc_relocate_f64(o, N, C.byref(o_new), C.byref(D))
        assert o_new.value == pytest.approx(-math.expm1(math.log1p(-o) / N), rel=1e-14)
        assert D.value == pytest.approx(ref.relocate_D(o_new.value, N), rel=1e-11)


def test_gate_and_noise_against_the_reference_at_the_gpu_bars():
    lib = _shim()
    o = np.array([0.0, 0.005, 0.004, 0.006, 0.5, 1.0], F32)
    g = np.zeros(len(o), F32)
    lib.hc_mcmc_gate(len(o), _p(o), _p(g))
    assert np.allclose(g, ref.gate(o.astype(np.float64)), rtol=1e-4, atol=1e-30) and g[-1] == 0 and abs(g[1] - 0.5) < 1e-5
    rng = np.random.default_rng(8)
    n = 20_000
    opacity = rng.normal(-5, 2, n).astype(F32)
    opacity[:10], opacity[10:20] = 20.0, -20.0
    scaling = rng.uniform(-7, 0, (n, 3)).astype(F32)
    rotation = (rng.normal(0, 1, (n, 4)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(F32)   # unnormalised
    noise = rng.standard_normal((n, 3)).astype(F32)
    noise[::9] = 0
    xyz = rng.normal(0, 3, (n, 3)).astype(F32)
    xyz[::18] = -0.0
    before = xyz.copy()
    lib.hc_mcmc_noise(n, _p(xyz), _p(opacity), _p(scaling), _p(rotation), _p(noise), 80.0)
    assert np.array_equal(xyz[::9].view(np.uint32), before[::9].view(np.uint32)), "a zero noise row leaves the bits of xyz"
    want = ref.noise_delta(opacity, scaling, rotation, noise, 80.0)
    # the displacement as the kernel formed it, before it was added to xyz: recomputed from xyz = 0
    zero = np.zeros((n, 3), F32)
    lib.hc_mcmc_noise(n, _p(zero), _p(opacity), _p(scaling), _p(rotation), _p(noise), 80.0)
    err, top = np.abs(zero - want), np.abs(want).max()
    assert top > 0 and err.max() <= 1e-4 * top and (err <= 1e-4 * np.abs(want) + 1e-6 * top).all()


def test_draw_search_and_ratio_clamp():
    lib = _shim()
    rng = np.random.default_rng(4)
    for relocate in (0, 1):
        n = 5000
        opacity = rng.normal(-4, 3, n).astype(F32)
        opacity[0] = opacity[-1] = -20.0   # dead rows at index 0 and at P - 1
        opacity[100:200] = -200.0          # sigmoid underflows to 0: weight 0 in either mode
        ref.keep_out_of_band(opacity, 0.005)
        w, dead, cdf, idx = np.zeros(n, F32), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32)
        pos = lib.hc_mcmc_weights(n, _p(opacity), 0.005, relocate, _p(w), _p(dead), _p(cdf), _p(idx))
        w_ref, dead_ref = ref.weights(opacity, 0.005, ref.RELOCATE if relocate else ref.GROW)
        assert np.array_equal(dead.astype(bool), dead_ref) and pos == int((w > 0).sum())
        assert relocate == 0 or (dead[0] and dead[-1] and dead.sum() > 500)
        u = np.concatenate([[0.0, np.nextafter(F32(1), F32(0))], rng.random(3000)]).astype(F32)
        sampled = np.zeros(len(u), np.int32)
        lib.hc_mcmc_draw(pos, _p(cdf), _p(idx), cdf[pos - 1], len(u), _p(u), _p(sampled))
        assert (w[sampled] > 0).all() and not dead[sampled].any(), "a row of weight zero was drawn"
        total = w_ref.sum()
        cdf_ref = np.cumsum(w_ref)
        t = u.astype(np.float64) * total
        lo = np.where(sampled > 0, cdf_ref[np.maximum(sampled - 1, 0)], 0.0)
        assert (t >= lo - 1e-6 * total).all() and (t <= cdf_ref[sampled] + 1e-6 * total).all()
        assert sampled[0] == np.flatnonzero(w > 0)[0], "u = 0 draws the first row of positive weight"
    # the search itself: first entry above t, on a cdf with ties and with a last-bit dip
    cdf = np.array([1.0, 1.0, 2.0, np.nextafter(2.0, 0.0), 5.0])
    idx = np.arange(5, dtype=np.int32)
    u = np.array([0.0, 0.19999999, 0.2, 0.5, 0.99999994], F32)
    out = np.zeros(5, np.int32)
    lib.hc_mcmc_draw(5, _p(cdf), _p(idx), 5.0, 5, _p(u), _p(out))
    assert out.tolist() == [0, 0, 2, 4, 4]
    assert [lib.hc_mcmc_ratio_clamp(r) for r in (1, 2, 51, 52, 60, 10 ** 6)] == [1, 2, 51, 51, 51, 51]


@pytest.mark.parametrize("name,extra", [("hostcheck_mcmc", ()),
                                        ("hostcheck_mcmc_san", ("-Xarch_host", "-fsanitize=address,undefined",
                                                                "-Xarch_host", "-fno-sanitize-recover=undefined"))])
def test_stand_alone_program_plain_and_sanitised(name, extra):
    """The shim's own main sweeps every function over its edge inputs.  The second build runs the host side under
    AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, never loaded into Python."""
    if not os.path.exists(hb.HIPCC):
        pytest.skip("no hipcc here")
    exe = os.path.join(HERE, "hostcheck_mcmc", name)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in [SRC] + hb._headers()):
        subprocess.check_call([hb.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", *hb.EXACT, "-DHOSTCHECK_MCMC_MAIN", *extra,
                               "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.startswith("checksum ") and out.stdout.strip().endswith("bad 0")


# ---- the ABI and the Python surface ----------------------------------------------------------------------------------------

def test_abi_rows_match_the_header():
    from diff_gaussian_rasterization import _C
    from tests import test_abi_table as abi
    protos, rows = abi.header_prototypes(), _C._ABI["required"][1]
    names = {"r3dgs_mcmc_workspace_bytes", "r3dgs_mcmc_noise", "r3dgs_mcmc_plan", "r3dgs_mcmc_move"}
    assert names == {n for n in protos if n.startswith("r3dgs_mcmc")} and names <= set(rows)
    for name in names:
        ret, kinds = protos[name]
        assert abi.ctypes_kind(rows[name][0]) == ret and [abi.ctypes_kind(t) for t in rows[name][1]] == kinds, name
    structs = abi.header_structs()
    assert [(f, abi.ctypes_kind(t)) for f, t in _C._McmcTensor._fields_] == structs["r3dgs_mcmc_tensor"] == structs["r3dgs_densify_tensor"]
    assert rows["r3dgs_mcmc_move"][1][6] is C.POINTER(_C._McmcTensor)
    lib = _C._lib
    assert lib.r3dgs_mcmc_workspace_bytes(0, 0) == 0 and lib.r3dgs_mcmc_workspace_bytes(-1, 5) == 0
    a, b = lib.r3dgs_mcmc_workspace_bytes(1000, 50), lib.r3dgs_mcmc_workspace_bytes(1000, 50)
    assert a == b and a >= 1000 * (8 + 4 + 16) and a % 16 == 0


def test_library_refuses_what_the_header_says():
    from diff_gaussian_rasterization import _C
    lib = _C._lib
    err = lambda: lib.r3dgs_last_error().decode()
    assert lib.r3dgs_mcmc_noise(10, None, None, None, None, None, 1.0, None) < 0 and "is NULL" in err()
    assert lib.r3dgs_mcmc_noise(0, None, None, None, None, None, 1.0, None) == 0
    assert lib.r3dgs_mcmc_plan(10, None, 0.005, 7, 0, None, None, None, None, None, None, None) < 0 and "unknown mode" in err()
    assert lib.r3dgs_mcmc_plan(10, None, 0.005, 0, 0, None, None, None, None, None, None, None) < 0 and "totals is NULL" in err()
    assert lib.r3dgs_mcmc_move(10, 0, 3, 0, 0.005, 0, None, None, None, None, None, None, None, None, None) < 0
    assert "n_new does not fit" in err()
    assert lib.r3dgs_mcmc_move(10, 1, 3, 0, 0.005, 40, None, None, None, None, None, None, None, None, None) < 0
    assert "R3DGS_MCMC_MAX_TENSORS" in err()
    assert lib.r3dgs_mcmc_move(10, 1, 0, 0, 0.005, 3, None, None, None, None, None, None, None, None, None) == 0   # nothing to add


def _host_model(P=6, M=4, step=True):
    import r3dgs_densify as dn
    s = densify_ref.random_state(P, M, seed=1)
    pc = types.SimpleNamespace()
    groups = []
    for name, attr in dn._GROUPS:
        p = torch.nn.Parameter(torch.from_numpy(s[name]))
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc._degrees = torch.from_numpy(s["degrees"])
    pc.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if step:
        for g in groups:
            g["params"][0].grad = torch.zeros_like(g["params"][0])
        pc.optimizer.step()
    return pc


def test_refusals():
    import r3dgs_mcmc as mc
    calls = {"inject_noise": lambda pc, **kw: mc.inject_noise(pc, 1.0, **kw), "relocate": lambda pc, **kw: mc.relocate(pc, **kw),
             "add_new": lambda pc, **kw: mc.add_new(pc, 100, **kw)}
    for what, call in calls.items():
        with pytest.raises(RuntimeError, match=f"{what}: the model has host tensors.*no CPU path"):
            call(_host_model())
        pc = _host_model()
        pc._scaling.data = pc._scaling.data.double()
        with pytest.raises(TypeError, match=f"{what}: pc._scaling is torch.float64, expected torch.float32"):
            call(pc)
        pc = _host_model()
        pc._rotation.data = torch.zeros(4, 6).t()
        with pytest.raises(ValueError, match=f"{what}: pc._rotation is not contiguous"):
            call(pc)
        pc = _host_model()
        pc._opacity.data = pc._opacity.data[:-1]
        with pytest.raises(ValueError, match=rf"{what}: pc._opacity has shape \(5, 1\), expected \[P, ...\] with P = 6"):
            call(pc)
    for what in ("relocate", "add_new"):
        pc = _host_model()
        pc._degrees = pc._degrees.long()
        with pytest.raises(TypeError, match=f"{what}: pc._degrees is torch.int64, expected torch.int32"):
            calls[what](pc)
        pc = _host_model()
        pc.optimizer.state[pc._xyz]["exp_avg"] = pc.optimizer.state[pc._xyz]["exp_avg"].double()
        with pytest.raises(TypeError, match=f"{what}: exp_avg of group 'xyz' is torch.float64"):
            calls[what](pc)
        pc = _host_model()
        pc.optimizer.state[pc._opacity]["exp_avg_sq"] = torch.zeros(7, 1)
        with pytest.raises(ValueError, match=f"{what}: exp_avg_sq of group 'opacity' has shape"):
            calls[what](pc)
        pc = _host_model()
        pc.optimizer.param_groups[0]["name"] = "means"
        with pytest.raises(ValueError, match="one single-parameter group per name"):
            calls[what](pc)
    with pytest.raises(ValueError, match=r"inject_noise: noise has shape \(5, 3\), expected \(P, 3\) with P = 6"):
        mc.inject_noise(_host_model(), 1.0, noise=torch.zeros(5, 3))
    with pytest.raises(TypeError, match="inject_noise: noise must be a torch.float32 tensor"):
        mc.inject_noise(_host_model(), 1.0, noise=torch.zeros(6, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="inject_noise: noise is not contiguous"):
        mc.inject_noise(_host_model(), 1.0, noise=torch.zeros(3, 6).t())
    with pytest.raises(ValueError, match=r"relocate: uniforms has shape \(5,\), expected \(P,\) with P = 6"):
        mc.relocate(_host_model(), uniforms=torch.zeros(5))
    with pytest.raises(TypeError, match="relocate: uniforms must be a torch.float32 tensor"):
        mc.relocate(_host_model(), uniforms=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"add_new: uniforms has shape \(6,\), expected \(n_new,\) with n_new = 2"):
        mc.add_new(_host_model(P=40), 1000, uniforms=torch.zeros(6))
    # nothing was changed by a refused call
    pc = _host_model()
    before, data = pc._xyz, pc._xyz.detach().clone()
    with pytest.raises(RuntimeError):
        mc.relocate(pc)
    assert pc._xyz is before and torch.equal(pc._xyz.detach(), data) and before in pc.optimizer.state


def test_strategy_schedule_and_regularisation():
    import r3dgs_mcmc as mc
    s = mc.MCMCStrategy(cap_max=1000)
    assert (s.noise_lr, s.refine_start, s.refine_stop, s.refine_every, s.min_opacity) == (5e5, 500, 25000, 100, 0.005)
    assert [i for i in range(0, 1001, 50) if s.is_refinement(i)] == [600, 700, 800, 900, 1000]
    assert not s.is_refinement(500) and not s.is_refinement(25000) and s.is_refinement(24900)
    pc = _host_model()
    want = 0.01 * torch.sigmoid(pc._opacity).mean() + 0.01 * torch.exp(pc._scaling).mean()
    got = mc.regularisation(pc)
    assert torch.allclose(got, want) and got.requires_grad
    assert torch.allclose(mc.regularisation(pc, 0.5, 0.0), 0.5 * torch.sigmoid(pc._opacity).mean())
