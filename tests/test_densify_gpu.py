"""GPU tests (-m gpu) of densification (reduced-3dgs_amd/r3dgs_densify.py, csrc/densify.hip).  The yardstick is
tests/densify_ref.py run on CPU copies of the same tensors with the same noise: everything that is a move is held bit for bit
(parameters, exp_avg, exp_avg_sq, stored grads, _degrees, the accumulators, the statistics, state['step']); the children's
positions and scales are held to the bounds derived there; the decisions are exact because the inputs keep out of the
ambiguity bands derived there (asserted)."""
import math
import types

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import densify_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
SCAN_SPAN = 256 * 256   # csrc/densify.hip: kScanSpan plan workgroups of kBlock Gaussians per round of the scan workgroup
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _make_optimizer(kind, groups):
    import r3dgs_optim
    if kind == "torch":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    return r3dgs_optim.Adam(groups, lr=0.0, eps=1e-15, capturable=kind == "r3dgs_capturable")


def _model(state, kind="torch", step=7.0):
    """A GaussianModel-shaped object on the device from a densify_ref state; optimizer state as after `step` steps."""
    pc = types.SimpleNamespace(percent_dense=ref.PERCENT_DENSE, max_sh_degree=3, active_sh_degree=3)
    groups = []
    for i, (name, attr) in enumerate(ATTRS.items()):
        p = torch.nn.Parameter(_dev(state[name]))
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3 * (i + 1), "name": name})
    pc._degrees = _dev(state["degrees"])
    for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
        setattr(pc, key, _dev(state[key]))
    pc.optimizer = _make_optimizer(kind, groups)
    if "exp_avg" in state:
        for g in groups:
            p, name = g["params"][0], g["name"]
            count = torch.tensor(step, dtype=torch.float32, device="cuda" if kind == "r3dgs_capturable" else "cpu")
            pc.optimizer.state[p] = {"step": count, "exp_avg": _dev(state["exp_avg"][name]),
                                     "exp_avg_sq": _dev(state["exp_avg_sq"][name])}
            if "grad" in state:
                p.grad = _dev(state["grad"][name])
    return pc


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == F32 else a


def _same_bits(t, want):
    want = np.asarray(want)
    return tuple(t.shape) == want.shape and np.array_equal(_bits(t), want.view(np.uint32) if want.dtype == F32 else want)


def _assert_equals_restatement(pc, out, store_grads, compacted):
    new = out["nA"] + out["nB"]
    assert pc._xyz.shape[0] == out["P"]
    for name, attr in ATTRS.items():
        p = getattr(pc, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_contiguous()
        if name in ("xyz", "scaling") and out["nC"]:
            assert _same_bits(p[:new], out[name][:new]), name
            got = p[new:].detach().cpu().numpy().astype(np.float64)
            err = np.abs(got - out[f"{name}_child64"]) / out[f"{name}_child_bound"]
            print(f"{name}_child: max error / bound = {err.max():.3f}")
            assert (err <= 1).all(), (name, float(err.max()))
        else:
            assert _same_bits(p, out[name]), name
        if "exp_avg" in out:
            state = pc.optimizer.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                assert _same_bits(state[key], out[key][name]), (key, name)
                assert not state[key][out["nA"]:].any()
            if store_grads:
                assert _same_bits(p.grad, out["grad"][name]) and not p.grad[out["nA"]:].any()
            else:
                assert p.grad is None
    assert _same_bits(pc._degrees, out["degrees"])
    keys = ("xyz_gradient_accum", "denom", "max_radii2D") + (() if compacted else ("density_gradient_accum",))
    for key in keys:
        assert _same_bits(getattr(pc, key), out[key]), key


def _assert_handed_over(pc, old_states, step):
    assert len(pc.optimizer.state) == len(ATTRS)
    for group in pc.optimizer.param_groups:
        p = group["params"][0]
        assert p is getattr(pc, ATTRS[group["name"]]) and len(group["params"]) == 1
        assert pc.optimizer.state[p] is old_states[group["name"]], "the state dict object is kept"
        assert float(pc.optimizer.state[p]["step"]) == step


def _band_free(P, M, seed, thr, densify=True, **kw):
    state = ref.keep_out_of_bands(ref.random_state(P, M, seed, **kw), thr, densify)
    assert not ref.in_band(state, thr, densify).any(), "a condition on the inputs: no row may sit in an ambiguity band"
    return state


@pytest.mark.parametrize("sh_degree", [0, 3])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 20_001, SCAN_SPAN + 1, 2 * SCAN_SPAN + 1])
def test_densify_and_prune_equals_the_restatement(P, sh_degree):
    import r3dgs_densify as dn
    M = (sh_degree + 1) ** 2
    screen = 20 if P % 2 else None
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, screen, ref.PERCENT_DENSE)
    state = _band_free(P, M, seed=P + sh_degree, thr=thr, grads=True)
    noise = np.random.default_rng(P).standard_normal((2, P, 3)).astype(F32)
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, screen, ref.PERCENT_DENSE, noise)
    runs = []
    for _ in range(2 if P == 20_001 else 1):
        pc = _model(state)
        old_states = {g["name"]: pc.optimizer.state[g["params"][0]] for g in pc.optimizer.param_groups}
        stats = {}
        dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, screen, stats, store_grads=True, noise=_dev(noise))
        assert stats == {k: out[k] for k in ("n_points_cloned", "n_points_split", "n_points_pruned")}
        assert all(type(v) is int for v in stats.values())
        _assert_equals_restatement(pc, out, store_grads=True, compacted=False)
        _assert_handed_over(pc, old_states, 7.0)
        runs.append([_bits(getattr(pc, a)) for a in ATTRS.values()])
    if P >= 20_001:
        assert out["nB"] > 100 and out["nC"] > 100 and out["n_points_pruned"] > 100 and out["nA"] < P
    for a, b in zip(runs[0], runs[-1]):
        assert np.array_equal(a, b), "not bit-identical from run to run"


def _four_bytes_off(t):
    """The same values in a contiguous view whose storage starts 4 bytes past a 16-byte boundary."""
    view = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def test_sources_four_bytes_off_a_sixteen_byte_boundary_move_word_by_word():
    """A parameter and a moment whose bases are not 16-byte aligned: their units are assembled from 4-byte loads
    (csrc/densify.hip move_kernel, src_vec == 0) and stored as 16 bytes.  Held to the restatement bit for bit."""
    import r3dgs_densify as dn
    P, M = 65, 16
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, ref.PERCENT_DENSE)
    state = _band_free(P, M, seed=P + 3, thr=thr, grads=True)
    noise = np.random.default_rng(P).standard_normal((2, P, 3)).astype(F32)
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, ref.PERCENT_DENSE, noise)
    assert out["nA"] > 0 and out["nB"] > 0 and out["nC"] > 0, "every segment has rows"
    pc = _model(state)
    with torch.no_grad():
        pc._features_rest.data = _four_bytes_off(pc._features_rest.data)          # 45-word rows
        moments = pc.optimizer.state[pc._xyz]
        moments["exp_avg"] = _four_bytes_off(moments["exp_avg"])                  # 3-word rows
    old_states = {g["name"]: pc.optimizer.state[g["params"][0]] for g in pc.optimizer.param_groups}
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, {}, store_grads=True, noise=_dev(noise))
    _assert_equals_restatement(pc, out, store_grads=True, compacted=False)
    _assert_handed_over(pc, old_states, 7.0)


def test_drawn_noise_is_seeded_by_the_generator_and_reads_only_split_parents():
    import r3dgs_densify as dn
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE)
    P = 5001
    state = _band_free(P, 16, seed=3, thr=thr)
    gen = torch.Generator(device="cuda").manual_seed(9)
    noise = torch.randn((2, P, 3), generator=gen, device="cuda")
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE, noise.cpu().numpy())
    pc = _model(state)
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, {}, generator=gen.manual_seed(9))
    _assert_equals_restatement(pc, out, store_grads=False, compacted=False)
    # NaN in the noise rows of Gaussians that are not split reaches nothing
    split = np.zeros(P, bool)
    split[out["src"][out["nA"] + out["nB"]:]] = True
    poisoned = noise.clone()
    poisoned[:, torch.from_numpy(~split).cuda()] = float("nan")
    pc2 = _model(state)
    dn.densify_and_prune(pc2, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, {}, noise=poisoned)
    assert torch.equal(pc2._xyz, pc._xyz) and torch.isfinite(pc2._xyz).all()


@pytest.mark.parametrize("P", [65, 20_001, SCAN_SPAN + 1])
def test_prune_points_equals_the_boolean_index_lines(P):
    import r3dgs_densify as dn
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE)
    state = ref.random_state(P, 16, seed=P, grads=True)
    pc = _model(state)
    mask = torch.rand(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(P)) < 0.3
    keep = ~mask
    want = {a: getattr(pc, a).detach()[keep] for a in ATTRS.values()}                        # gaussian_model.py:513
    for a in ATTRS.values():
        st = pc.optimizer.state[getattr(pc, a)]
        want[a + ".exp_avg"], want[a + ".exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]   # :507-508
        want[a + ".grad"] = getattr(pc, a).grad[keep]                                        # :512
    for key in ("_degrees", "xyz_gradient_accum", "denom", "max_radii2D"):                  # :563-568
        want[key] = getattr(pc, key)[keep]
    old_states = {g["name"]: pc.optimizer.state[g["params"][0]] for g in pc.optimizer.param_groups}
    dn.prune_points(pc, mask, store_grads=True)
    for a in ATTRS.values():
        p = getattr(pc, a)
        st = pc.optimizer.state[p]
        assert torch.equal(p.detach(), want[a]) and torch.equal(st["exp_avg"], want[a + ".exp_avg"])
        assert torch.equal(st["exp_avg_sq"], want[a + ".exp_avg_sq"]) and torch.equal(p.grad, want[a + ".grad"])
    for key in ("_degrees", "xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(pc, key), want[key]) and getattr(pc, key).shape == want[key].shape, key
    _assert_handed_over(pc, old_states, 7.0)
    _assert_equals_restatement(pc, ref.prune_points(state, mask.cpu().numpy()), store_grads=True, compacted=True)
    del thr


@pytest.mark.parametrize("max_screen_size", [None, 20])
def test_prune_alone_sees_max_radii2D_and_densify_does_not(max_screen_size):
    import r3dgs_densify as dn
    P = 20_001
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, max_screen_size, ref.PERCENT_DENSE)
    state = _band_free(P, 4, seed=8, thr=thr, densify=False)
    assert (state["max_radii2D"] > 20).sum() > 1000     # non-zero radii: the screen-size term has something to act on
    out = ref.prune(state, ref.MIN_OPACITY, ref.EXTENT, max_screen_size)
    pc = _model(state)
    stats = {}
    dn.prune(pc, ref.MIN_OPACITY, ref.EXTENT, max_screen_size, stats)
    assert stats == {"n_points_pruned": out["n_points_pruned"]}
    _assert_equals_restatement(pc, out, store_grads=False, compacted=True)
    if max_screen_size:
        big = state["max_radii2D"] > 20
        assert not big[out["src"]].any(), "the screen-size term acted"
        # the quirk: inside densify_and_prune the same Gaussians survive, max_radii2D has been zeroed by then
        state2 = _band_free(P, 4, seed=8, thr=thr)
        out2 = ref.densify_and_prune(state2, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, ref.PERCENT_DENSE,
                                     np.zeros((2, P, 3), F32))
        assert (state2["max_radii2D"] > 20)[out2["src"]].sum() > 500
        pc2 = _model(state2)
        dn.densify_and_prune(pc2, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, {}, noise=torch.zeros(2, P, 3, device="cuda"))
        _assert_equals_restatement(pc2, out2, store_grads=False, compacted=False)


@pytest.mark.parametrize("kind", ["torch", "r3dgs", "r3dgs_capturable"])
def test_optimizer_hand_over(kind):
    """After densify_and_prune one optimizer.step() with fixed grads gives the bits of stepping an optimizer of the same
    class that was handed the restatement's state (and the device's parameters)."""
    import r3dgs_densify as dn
    P = 3001
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE)
    state = _band_free(P, 16, seed=21, thr=thr)
    noise = np.random.default_rng(4).standard_normal((2, P, 3)).astype(F32)
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE, noise)
    pc = _model(state, kind)
    old_states = {g["name"]: pc.optimizer.state[g["params"][0]] for g in pc.optimizer.param_groups}
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, {}, noise=_dev(noise))
    _assert_handed_over(pc, old_states, 7.0)
    twin_state = dict(out, **{n: getattr(pc, a).detach().cpu().numpy() for n, a in ATTRS.items()})
    twin_state.update(xyz_gradient_accum=np.zeros((out["P"], 1), F32), denom=np.zeros((out["P"], 1), F32))
    twin = _model(twin_state, kind)
    rng = np.random.default_rng(6)
    for name, attr in ATTRS.items():
        g = _dev(rng.normal(0, 1e-3, twin_state[name].shape).astype(F32))
        getattr(pc, attr).grad, getattr(twin, attr).grad = g, g.clone()
    pc.optimizer.step()
    twin.optimizer.step()
    for attr in ATTRS.values():
        a, b = getattr(pc, attr), getattr(twin, attr)
        assert torch.equal(a.detach(), b.detach()), attr
        sa, sb = pc.optimizer.state[a], twin.optimizer.state[b]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
        assert float(sa["step"]) == float(sb["step"]) == 8.0


def test_a_group_without_state_moves_its_parameter_only():
    import r3dgs_densify as dn
    P = 1000
    thr = ref.thresholds(ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE)
    state = _band_free(P, 16, seed=13, thr=thr, moments=False)
    noise = np.zeros((2, P, 3), F32)
    out = ref.densify_and_prune(state, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, ref.PERCENT_DENSE, noise)
    pc = _model(state)
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, {}, store_grads=True, noise=_dev(noise))
    assert len(pc.optimizer.state) == 0
    _assert_equals_restatement(pc, out, store_grads=False, compacted=False)


class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


class _PipeExact(_Pipe):
    debug = True


class _Cam:
    def __init__(self, c, W, H):
        self.FoVx, self.FoVy = 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy)
        self.image_height, self.image_width = H, W
        self.world_view_transform, self.full_proj_transform = _dev(c.world_view_transform), _dev(c.full_proj_transform)
        self.camera_center = _dev(c.camera_center)


def test_empty_model_in_and_out_and_a_render_of_nothing():
    import r3dgs_densify as dn
    import r3dgs_render
    empty = ref.random_state(0, 16, seed=0)
    pc = _model(empty)
    stats = {}
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, 20, stats)
    assert stats == {"n_points_cloned": 0, "n_points_split": 0, "n_points_pruned": 0} and pc._xyz.shape == (0, 3)
    dn.prune_points(pc, torch.zeros(0, dtype=torch.bool, device="cuda"))
    assert pc._features_rest.shape == (0, 15, 3) and len(pc.optimizer.state) == 6
    state = ref.random_state(777, 16, seed=5)
    state["opacity"][:] = -12.0                     # sigmoid = 6e-6: everything is pruned
    pc = _model(state)
    dn.densify_and_prune(pc, ref.MAX_GRAD, ref.MIN_OPACITY, ref.EXTENT, None, stats)
    assert pc._xyz.shape == (0, 3) and pc._degrees.shape[0] == 0 and pc.denom.shape == (0, 1)
    assert stats["n_points_pruned"] == 777 + stats["n_points_cloned"] + stats["n_points_split"]
    cam = _Cam(ss.make_camera(64, 64, 60.0, 1), 64, 64)
    bg = _dev(np.array([0.1, 0.2, 0.3], F32))
    out = r3dgs_render.render(cam, pc, _Pipe, bg)     # the empty model renders without error
    assert out["render"].shape == (3, 64, 64) and torch.isfinite(out["render"]).all() and out["radii"].shape == (0,)


def test_thirty_step_loop_with_densification_every_ten_steps():
    """The shape of test_train_loop_gpu.py's loop with the real call instead of its stand-in: it runs, the Gaussian count
    changes, and every consumed pass (default settings) equals the exact-size path bit for bit."""
    import r3dgs_densify as dn
    import r3dgs_render
    from r3dgs_train_stats import add_densification_stats
    W = H = 64
    P0 = 3000
    base = ss.make_camera(W, H, 60.0, None)
    g = ss.make_gaussians(P0, base, seed=31, degree_mode="mixed", scale_mu=0.05, zmin=2.0, zmax=8.0)
    cams = [_Cam(ss.make_camera(W, H, 60.0, k), W, H) for k in range(4)]
    bg = _dev(np.array([0.1, 0.2, 0.3], F32))
    state = {"xyz": g["means3D"], "f_dc": g["sh"][:, :1], "f_rest": g["sh"][:, 1:], "opacity": g["opacity"],   # raw already
             "scaling": np.log(g["scales"]).astype(F32), "rotation": g["rotations"],
             "degrees": g["degrees"], "xyz_gradient_accum": np.zeros((P0, 1), F32),
             "denom": np.zeros((P0, 1), F32), "max_radii2D": np.zeros(P0, F32)}
    state = {k: np.ascontiguousarray(v) for k, v in state.items()}
    pc = _model(state, "r3dgs")
    with torch.no_grad():
        targets = [r3dgs_render.render(c, pc, _PipeExact, bg)["render"].clone() for c in cams]
        pc._xyz.add_(0.02 * torch.randn(pc._xyz.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)))
    leaves = list(ATTRS.values())
    counts, gen = [P0], torch.Generator(device="cuda").manual_seed(2)
    for step in range(30):
        k = step % len(cams)
        pc.optimizer.zero_grad(set_to_none=True)
        out = r3dgs_render.render(cams[k], pc, _Pipe, bg)
        (out["render"] - targets[k]).abs().mean().backward()
        got = [getattr(pc, a).grad.clone() for a in leaves]
        for a in leaves:
            getattr(pc, a).grad = None
        exact = r3dgs_render.render(cams[k], pc, _PipeExact, bg)
        (exact["render"] - targets[k]).abs().mean().backward()
        assert torch.equal(out["render"], exact["render"]) and torch.equal(out["radii"], exact["radii"]), step
        assert torch.equal(out["viewspace_points"].grad, exact["viewspace_points"].grad), step
        for a, grad in zip(leaves, got):
            assert torch.equal(grad, getattr(pc, a).grad) and torch.isfinite(grad).all(), (step, a)
        add_densification_stats(pc, out["viewspace_points"], out["radii"])
        pc.optimizer.step()
        if step % 10 == 9:
            grads = (pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0, posinf=0.0)
            max_grad = max(float(grads.quantile(0.9)), 1e-12)
            stats = {}
            dn.densify_and_prune(pc, max_grad, ref.MIN_OPACITY, ref.EXTENT, None, stats, generator=gen)
            counts.append(pc._xyz.shape[0])
            assert stats["n_points_cloned"] + stats["n_points_split"] > 0
            assert not pc.xyz_gradient_accum.any() and pc.denom.shape == (counts[-1], 1)
    print(f"\ndensify loop: P {counts}")
    assert len(set(counts)) > 1, "the Gaussian count never changed"
