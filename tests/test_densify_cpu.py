"""CPU checks of densification (reduced-3dgs_amd/r3dgs_densify.py, csrc/densify.hip, csrc/densify_math.h,
include/r3dgs_densify.h): the per-Gaussian kernel arithmetic runs on the host through a test shim and must take the decisions
of the numpy restatement (tests/densify_ref.py) exactly on inputs that keep out of the ambiguity bands derived there; the
children's positions equal a float32 numpy restatement bit for bit and their scales stay within the derived bound; the
restatement's segment order equals a literal cat / mask / cat / mask / mask; the Python surface refuses what the kernels do not
take.  No GPU needed."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import r3dgs_densify as dn
from tests import densify_ref as ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_densify", "hostcheck_densify.hip")
SO = os.path.join(HERE, "hostcheck_densify", "libhostcheck_densify.so")
F32 = np.float32
CLONE, SPLIT, PRUNED_SELF, PRUNED_CHILD = 1, 2, 4, 8   # csrc/densify_math.h kFlag*


def _shim():
    lib = build_shim(SRC, SO, EXACT, "hipcc not available to build the densification host-check shim")
    lib.hc_densify_flags.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float] + \
        [C.c_void_p] * 6
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _flags(lib, state, thr, densify):
    P = state["scaling"].shape[0]
    out = np.zeros(P, np.uint8)
    arrays = [np.ascontiguousarray(state[k], F32) for k in ("xyz_gradient_accum", "denom", "scaling", "opacity", "max_radii2D")]
    lib.hc_densify_flags(P, int(densify), float(thr["max_grad"]), float(thr["dense_scale"]), float(thr["min_opacity"]),
                         int(thr["screen"]), float(thr["max_screen"]), float(thr["world_scale"]), *(_p(a) for a in arrays),
                         _p(out))
    return out


def _assert_flags_equal(flags, d):
    assert np.array_equal((flags & CLONE) != 0, d["clone"])
    assert np.array_equal((flags & SPLIT) != 0, d["split"])
    assert np.array_equal((flags & PRUNED_SELF) != 0, d["pruned_self"])
    assert np.array_equal((flags & PRUNED_CHILD) != 0, d["pruned_child"])


@pytest.mark.parametrize("max_screen_size", [None, 20])
@pytest.mark.parametrize("densify", [True, False])
def test_flags_on_host_equal_the_restatement_on_band_free_inputs(densify, max_screen_size):
    lib = _shim()
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, max_screen_size, ref.PERCENT_DENSE)
    state = ref.keep_out_of_bands(ref.random_state(20_001, 4, seed=11 + densify), thr, densify)
    assert not ref.in_band(state, thr, densify).any(), "a condition on the inputs: no row may sit in an ambiguity band"
    d = ref.decisions(state, thr, densify)
    if densify:   # the mix the test is about
        assert d["clone"].sum() > 500 and d["split"].sum() > 500 and (d["pruned_child"].sum() > 20 or not max_screen_size)
    assert 100 < d["pruned_self"].sum() < 19_000
    _assert_flags_equal(_flags(lib, state, thr, densify), d)


def test_the_band_is_a_few_ulp_and_the_nudge_leaves_it():
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, ref.PERCENT_DENSE)
    assert ref.SCALE_BAND_REL < 3 * ref.U and ref.OPACITY_BAND_REL < 5 * ref.U and ref.child_world_band_rel(0.5) < 8 * ref.U
    state = ref.random_state(64, 4, seed=2)
    state["scaling"][:8] = F32(np.log(float(thr["dense_scale"])))    # on the threshold: inside the band
    state["scaling"][8:16] = F32(np.log(float(thr["world_scale"])))
    state["scaling"][16:24] = F32(np.log(1.6 * float(thr["world_scale"])))
    state["opacity"][24:32] = F32(np.log(0.005 / 0.995))
    assert ref.in_band(state, thr)[:32].all()
    assert not ref.in_band(ref.keep_out_of_bands(state, thr), thr).any()


def test_special_values():
    """denom == 0 with a zero accumulator (NaN -> 0: not selected) and with a positive one (inf: selected); negative zero;
    denormal gradients; raw scales of +-30; none of it may disturb a decision."""
    lib = _shim()
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE)
    accum = np.array([0, 1e-3, -0.0, 0.0, 1e-40, 3e-39, 1.0, 1.0, 2e-4, 1.9e-4, np.inf, 1.0], F32).reshape(-1, 1)
    denom = np.array([0, 0, 0, -0.0, 1, 1e-38, 1, 1, 1, 1, 1, np.inf], F32).reshape(-1, 1)
    n = len(accum)
    state = {"xyz_gradient_accum": accum, "denom": denom, "opacity": np.full((n, 1), 2.0, F32),
             "scaling": np.full((n, 3), -6.0, F32), "max_radii2D": np.zeros(n, F32)}
    state["scaling"][6] = 30.0
    state["scaling"][7] = -30.0
    g = np.zeros(n, F32)
    lib.hc_densify_grad(n, _p(accum), _p(denom), _p(g))
    want = ref.grads32(accum, denom)
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
    assert g[0] == 0 and np.isinf(g[1]) and g[2] == 0 and g[3] == 0 and np.isinf(g[10]) and g[11] == 0
    assert not ref.in_band(state, thr).any()
    d = ref.decisions(state, thr)
    flags = _flags(lib, state, thr, True)
    _assert_flags_equal(flags, d)
    hot = (flags & (CLONE | SPLIT)) != 0
    assert hot.tolist() == [False, True, False, False, False, True, True, True, True, False, True, False]
    assert flags[6] & SPLIT and flags[7] & CLONE


def test_child_rows_position_bit_for_bit_and_scale_within_the_derived_bound():
    lib = _shim()
    rng = np.random.default_rng(5)
    n = 30_000
    raw_q = (rng.normal(0, 1, (n, 4)) * 10.0 ** rng.uniform(-1, 1, (n, 1))).astype(F32)
    raw_q[:50] *= F32(1e-15)     # far below unit length, down to the clamp of the norm
    raw_q[50:100] *= F32(1e12)   # far above
    raw_q[100] = 0               # the zero quaternion: q = 0 / 1e-12
    raw_scale = rng.uniform(-8, 1, (n, 3)).astype(F32)
    raw_scale[200:210] = 30.0
    raw_scale[210:220] = -30.0
    noise = rng.standard_normal((n, 3)).astype(F32)
    xyz = rng.normal(0, 3, (n, 3)).astype(F32)
    scale = np.zeros((n, 3), F32)
    lib.hc_scale_act(3 * n, _p(raw_scale), _p(scale))
    assert (np.abs(scale.astype(np.float64) / np.exp(raw_scale.astype(np.float64)) - 1) <= ref.EXPF_REL).all()
    got = np.zeros((n, 3), F32)
    lib.hc_child_xyz(n, _p(raw_q), _p(scale), _p(noise), _p(xyz), _p(got))
    want = ref.child_xyz32(raw_q, scale, noise, xyz)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "xyz_child: not the stated operation order"
    assert np.isfinite(got).all()
    value, bound = ref.child_xyz64(raw_q, raw_scale, noise, xyz)
    assert (np.abs(got - value) <= bound).all(), float((np.abs(got - value) / bound).max())
    child = np.zeros((n, 3), F32)
    lib.hc_child_scaling(3 * n, _p(scale), _p(child))
    value, bound = ref.child_scaling64(raw_scale)
    assert (np.abs(child - value) <= bound).all(), float((np.abs(child - value) / bound).max())


def _brute_force(state, thr, noise):
    """The reference's sequence performed literally on numpy arrays: cat the clones, cat the children, mask out the parents,
    mask out the pruned.  Rows carry (source, kind) tags; kind 0 original, 1 clone, 2 / 3 first / second child."""
    P = state["scaling"].shape[0]
    scaling = state["scaling"].astype(np.float64)
    opacity = state["opacity"].reshape(-1).astype(np.float64)
    tag = np.stack([np.arange(P), np.zeros(P, int)], 1)
    grads = ref.grads32(state["xyz_gradient_accum"], state["denom"])
    dense, world = np.float64(thr["dense_scale"]), np.float64(thr["world_scale"])

    def smax(s):
        return np.exp(s).max(axis=1) if len(s) else np.zeros(0)
    clone = (grads >= thr["max_grad"]) & (smax(scaling) <= dense)                                  # :653-655
    n_cloned = int(clone.sum())
    scaling, opacity = np.concatenate([scaling, scaling[clone]]), np.concatenate([opacity, opacity[clone]])   # cat
    tag = np.concatenate([tag, np.stack([np.flatnonzero(clone), np.ones(n_cloned, int)], 1)])
    padded = np.zeros(len(scaling), F32)                                                           # :626-627
    padded[:P] = grads
    split = (padded >= thr["max_grad"]) & (smax(scaling) > dense)                                  # :628-630
    n_split = int(split.sum())
    child_scaling = np.tile(scaling[split] - np.log(np.float64(ref.CHILD_SHRINK)), (2, 1))        # repeat(N, 1)
    child_tag = np.stack([np.tile(tag[split][:, 0], 2), np.repeat([2, 3], n_split)], 1)
    scaling = np.concatenate([scaling, child_scaling])                                             # cat
    opacity = np.concatenate([opacity, np.tile(opacity[split], 2)])
    tag = np.concatenate([tag, child_tag])
    keep = ~np.concatenate([split, np.zeros(2 * n_split, bool)])                                   # :647-648
    scaling, opacity, tag = scaling[keep], opacity[keep], tag[keep]
    prune = 1.0 / (1.0 + np.exp(-opacity)) < np.float64(thr["min_opacity"])                        # :685
    if thr["screen"]:
        radii = np.zeros(len(scaling), F32)                                                        # zeroed by the postfix
        prune |= (radii > thr["max_screen"]) | (smax(scaling) > world)                             # :687-689
    return tag[~prune], n_cloned, n_split, int(prune.sum())


@pytest.mark.parametrize("case", ["mixed", "none", "all_cloned", "all_split", "all_pruned"])
@pytest.mark.parametrize("P", [0, 1, 2, 65, 1000])
def test_segment_order_and_offsets_against_the_literal_sequence(P, case):
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20 if case in ("mixed", "all_pruned") else None,
                         ref.PERCENT_DENSE)
    state = ref.random_state(P, 4, seed=P)
    if case != "mixed":
        state["opacity"][:] = -12.0 if case == "all_pruned" else 3.0
        state["denom"][:] = 1
        state["xyz_gradient_accum"][:] = 0.0 if case == "none" else 1.0
        state["scaling"][:] = {"all_split": -1.0}.get(case, -7.0)
    ref.keep_out_of_bands(state, thr)
    assert not ref.in_band(state, thr).any()
    noise = np.random.default_rng(1).standard_normal((2, P, 3)).astype(F32)
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20 if thr["screen"] else None,
                                ref.PERCENT_DENSE, noise)
    tag, n_cloned, n_split, n_pruned = _brute_force(state, thr, noise)
    assert (out["n_points_cloned"], out["n_points_split"], out["n_points_pruned"]) == (n_cloned, n_split, n_pruned)
    kind = np.concatenate([np.zeros(out["nA"], int), np.ones(out["nB"], int), np.full(out["nC"], 2), np.full(out["nC"], 3)])
    assert out["P"] == len(tag) == len(kind)
    assert np.array_equal(out["src"], tag[:, 0]) and np.array_equal(kind, tag[:, 1])
    if P:
        assert {"none": out["P"] == P, "all_cloned": out["nB"] == P and out["nA"] == P, "all_pruned": out["P"] == 0,
                "all_split": out["nC"] == P and out["nA"] == 0, "mixed": True}[case]
    # moved rows are moves: the moments follow in A and are zero elsewhere
    for name in ref.NAMES:
        assert np.array_equal(out["exp_avg"][name][:out["nA"]], state["exp_avg"][name][out["src"][:out["nA"]]])
        assert not out["exp_avg_sq"][name][out["nA"]:].any()
    assert np.array_equal(out["degrees"], state["degrees"][out["src"]])


# ---- the Python surface ------------------------------------------------------------------------------------------------------

def _host_model(P=6, M=4, step=True):
    s = ref.random_state(P, M, seed=1)
    pc = types.SimpleNamespace(percent_dense=ref.PERCENT_DENSE)
    groups = []
    for name, attr in dn._GROUPS:
        p = torch.nn.Parameter(torch.from_numpy(s[name]))
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc._degrees = torch.from_numpy(s["degrees"])
    pc.xyz_gradient_accum, pc.denom = torch.from_numpy(s["xyz_gradient_accum"]), torch.from_numpy(s["denom"])
    pc.max_radii2D = torch.from_numpy(s["max_radii2D"])
    pc.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if step:
        for g in groups:
            g["params"][0].grad = torch.zeros_like(g["params"][0])
        pc.optimizer.step()
    return pc


def _call(pc, **kw):
    dn.densify_and_prune(pc, kw.pop("max_grad", ref.MAX_GRAD), ref.MIN_OPACITY, ref.EXTENT, None, {}, **kw)


def test_refusals():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call(_host_model())
    with pytest.raises(RuntimeError, match="no CPU path"):
        dn.prune(_host_model(), ref.MIN_OPACITY, ref.EXTENT, 20, {})
    with pytest.raises(RuntimeError, match="no CPU path"):
        dn.prune_points(_host_model(), torch.zeros(6, dtype=torch.bool))
    for bad in (0.0, -1e-4, float("nan")):
        with pytest.raises(ValueError, match="max_grad.*must be > 0.*split the clones"):
            _call(_host_model(), max_grad=bad)
    pc = _host_model()
    pc._features_rest.data = pc._features_rest.data.transpose(1, 2).contiguous().transpose(1, 2)
    with pytest.raises(ValueError, match="_features_rest is not contiguous"):
        _call(pc)
    pc = _host_model()
    pc._degrees = pc._degrees.long()
    with pytest.raises(TypeError, match="_degrees is torch.int64, expected torch.int32"):
        _call(pc)
    pc = _host_model()
    pc.optimizer.state[pc._xyz]["exp_avg"] = pc.optimizer.state[pc._xyz]["exp_avg"].double()
    with pytest.raises(TypeError, match="exp_avg of group 'xyz' is torch.float64"):
        _call(pc)
    pc = _host_model()
    pc.denom = pc.denom[:-1]
    with pytest.raises(ValueError, match=r"pc.denom has shape \(5, 1\), expected \[P, ...\] with P = 6"):
        _call(pc)
    pc = _host_model()
    pc.optimizer.state[pc._opacity]["exp_avg_sq"] = torch.zeros(7, 1)
    with pytest.raises(ValueError, match="exp_avg_sq of group 'opacity' has shape"):
        _call(pc)
    with pytest.raises(ValueError, match=r"noise has shape \(2, 5, 3\), expected \(2, P, 3\) with P = 6"):
        _call(_host_model(), noise=torch.zeros(2, 5, 3))
    with pytest.raises(TypeError, match="noise must be a torch.float32 tensor"):
        _call(_host_model(), noise=torch.zeros(2, 6, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="noise is not contiguous"):
        _call(_host_model(), noise=torch.zeros(3, 6, 2).permute(2, 1, 0))
    with pytest.raises(ValueError, match=r"mask has shape \(5,\)"):
        dn.prune_points(_host_model(), torch.zeros(5, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask must be a torch.bool tensor"):
        dn.prune_points(_host_model(), torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="store_grads=True but pc._xyz has no .grad"):
        pc = _host_model()
        pc._xyz.grad = None
        _call(pc, store_grads=True)
    pc = _host_model()
    pc.optimizer.param_groups[0]["name"] = "means"
    with pytest.raises(ValueError, match="one single-parameter group per name"):
        _call(pc)
    # nothing was changed by a refused call
    pc = _host_model()
    before = pc._xyz
    with pytest.raises(RuntimeError):
        _call(pc)
    assert pc._xyz is before and pc.optimizer.param_groups[0]["params"][0] is before and before in pc.optimizer.state


def test_library_refuses_what_the_header_says():
    lib = dn._lib
    lib.r3dgs_last_error.restype = C.c_char_p
    assert lib.r3dgs_densify_workspace_bytes(0) == 0 and lib.r3dgs_densify_workspace_bytes(-3) == 0
    nb = (1000 + 255) // 256
    assert lib.r3dgs_densify_workspace_bytes(1000) >= 64 + 1000 + 4 * 8 * nb + 8 * 1000
    assert lib.r3dgs_densify_plan(10, 1, None, None, None, None, None, 0.0, 1.0, 0.1, 0, 0.0, 1.0, None, None, None) < 0
    assert b"max_grad must be > 0" in lib.r3dgs_last_error()
    assert lib.r3dgs_densify_move(10, 11, 0, 0, 0, None, None, None, None, None, None, None) < 0
    assert b"do not fit" in lib.r3dgs_last_error()
    assert lib.r3dgs_densify_move(10, 5, 5, 5, 40, None, None, None, None, None, None, None) < 0
    assert b"R3DGS_DENSIFY_MAX_TENSORS" in lib.r3dgs_last_error()
