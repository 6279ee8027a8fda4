"""GPU tests (-m gpu) of the 3DGS-MCMC strategy (reduced-3dgs_amd/r3dgs_mcmc.py, csrc/mcmc.hip).  The yardstick is
tests/mcmc_ref.py run on CPU copies of the same tensors with the same noise and uniforms.

Draws: for every draw u * total lies in [cdf_ref[j-1] - tol, cdf_ref[j] + tol], tol = 1e-6 * total (the device's fp32 sigmoid is
not bit-reproducible on the host), and no dead or zero-weight row is ever drawn (exact).  Everything downstream is held to the
reference FED THE DEVICE'S OWN `sampled`: slots, ratio, totals and every moved row -- copies and zeros bit for bit (parameters
that were not updated, moments, _degrees, accumulators, state['step'], the identity of untouched tensor objects), the updated
opacity / scaling rows within the per-element bound mcmc_ref.py derives (inputs keep sigmoid(opacity) <= 0.99).
Noise: the displacement against the float64 reference, max error <= 1e-4 max|ref| and per element |err| <= 1e-4 |ref| + 1e-6
max|ref|, on every element.  Measured worst figures: profiles/mcmc_gpu_tests.txt."""
import math

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import densify_ref
from tests import mcmc_ref as ref
from tests.test_densify_gpu import ATTRS, _Cam, _Pipe, _bits, _dev, _model

pytestmark = pytest.mark.gpu

F32 = np.float32
SCAN_SPAN = 256 * 256   # csrc/mcmc.hip: kScanSpan plan workgroups of kBlock Gaussians per round of the scan workgroup
MIN_OPACITY = 0.005
MAX_SIGMOID = 0.99
BELOW_ONE = np.nextafter(F32(1), F32(0))


def _state(P, seed, moments=True):
    s = densify_ref.random_state(P, 4, seed, moments=moments)
    s["opacity"] = np.minimum(s["opacity"], F32(math.log(MAX_SIGMOID / (1 - MAX_SIGMOID)) - 1e-3))
    ref.keep_out_of_band(s["opacity"], MIN_OPACITY)
    assert not ref.in_band(s["opacity"], MIN_OPACITY).any() and (ref.sigmoid64(s["opacity"]) <= MAX_SIGMOID).all()
    return s


def _snapshot(pc):
    """Every tensor object of the model and its optimizer state, by name."""
    objs = {}
    for name, attr in ATTRS.items():
        p = getattr(pc, attr)
        objs[name] = p
        st = pc.optimizer.state.get(p)
        if st is not None:
            objs[name + ".state"] = st
            objs[name + ".exp_avg"], objs[name + ".exp_avg_sq"], objs[name + ".step"] = st["exp_avg"], st["exp_avg_sq"], st["step"]
    objs["degrees"] = pc._degrees
    for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
        objs[key] = getattr(pc, key)
    return objs


def _same(t, want):
    want = np.asarray(want)
    got = _bits(t)
    return tuple(t.shape) == want.shape and np.array_equal(got, want.view(np.uint32) if want.dtype == F32 else want)


def _check_plan(opacity, mode, uniforms, stats, n_want):
    """The plan's outputs against the reference -> (sampled, slots, ratio) as the device made them."""
    P = len(opacity)
    totals = stats["totals"].cpu().numpy()
    w, dead = ref.weights(opacity, MIN_OPACITY, mode)
    n = int(totals[1])
    sampled = stats["sampled"].cpu().numpy()[:n].astype(np.int64)
    ratio = stats["ratio"].cpu().numpy()
    slots = stats["slots"].cpu().numpy()[:n].astype(np.int64) if mode == ref.RELOCATE else None
    assert totals.tolist() == ref.plan_totals(w, dead, mode, n_want, sampled)
    if mode == ref.RELOCATE:
        assert np.array_equal(slots, np.flatnonzero(dead)[:n]), "slots: the dead rows in index order"
    if n:
        assert ((sampled >= 0) & (sampled < P)).all()
        assert not dead[sampled].any() and (w[sampled] > 0).all(), "a dead or zero-weight row was drawn"
        cdf = np.cumsum(w)
        total = cdf[-1]
        t = np.asarray(uniforms, np.float64)[:n] * total
        lo = np.where(sampled > 0, cdf[np.maximum(sampled - 1, 0)], 0.0)
        assert (t >= lo - 1e-6 * total).all() and (t <= cdf[sampled] + 1e-6 * total).all(), "a draw outside its band"
    assert np.array_equal(ratio, ref.ratio_of(P, sampled)[0]) and ratio.dtype == np.int32
    return sampled, slots, ratio


def _check_updated(pc, state, out, upd, copies, bounded=None):
    """Opacity and scaling: rows outside `upd` and `copies` bit for bit, the drawn sources within the bound, and the copies
    (destination -> source pairs) bit-equal to the source's row on the device.  -> worst error / bound."""
    worst = 0.0
    for name, col in (("opacity", 0), ("scaling", 1)):
        got = getattr(pc, ATTRS[name]).detach().cpu().numpy()
        loose = np.zeros(got.shape[0], bool)
        loose[list(upd)] = True
        loose[copies[0]] = True
        assert np.array_equal(got[~loose].view(np.uint32), out[name][~loose].view(np.uint32)), name
        assert np.isfinite(got).all()
        assert np.array_equal(got[copies[0]].view(np.uint32), got[copies[1]].view(np.uint32)), f"{name}: a copy differs from its source"
        for i, row in upd.items():
            if bounded is not None and not bounded[i]:
                continue
            err = np.abs(got[i].astype(np.float64) - np.atleast_1d(row[col])) / np.atleast_1d(row[2 + col])
            worst = max(worst, float(err.max()))
    assert worst <= 1.0, f"an updated row misses the derived bound: {worst}"
    return worst


def _relocate_and_check(state, kind, zero_relocated, uniforms, bounded=None):
    import r3dgs_mcmc as mc
    P = state["xyz"].shape[0]
    pc = _model(state, kind)
    before = _snapshot(pc)
    stats = mc.relocate(pc, MIN_OPACITY, uniforms=_dev(uniforms), zero_relocated=zero_relocated)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in stats.values())
    sampled, slots, ratio = _check_plan(state["opacity"].reshape(-1), ref.RELOCATE, uniforms, stats, None)
    out, upd = ref.relocate(state, sampled, slots, ratio, MIN_OPACITY, zero_relocated)
    after = _snapshot(pc)
    assert after.keys() == before.keys() and all(after[k] is before[k] for k in before), "relocation replaces no tensor object"
    for name, attr in ATTRS.items():
        if name not in ("opacity", "scaling"):
            assert _same(getattr(pc, attr), out[name]), name
        if "exp_avg" in state:
            st = pc.optimizer.state[getattr(pc, attr)]
            assert _same(st["exp_avg"], out["exp_avg"][name]) and _same(st["exp_avg_sq"], out["exp_avg_sq"][name]), name
            assert float(st["step"]) == 7.0
    assert "exp_avg" in state or len(pc.optimizer.state) == 0
    assert _same(pc._degrees, out["degrees"])
    for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert _same(getattr(pc, key), state[key]), key
    worst = _check_updated(pc, state, out, upd, (slots, sampled), bounded)
    return pc, stats, worst, len(sampled)


@pytest.mark.parametrize("P,kind,zero_relocated,moments", [(1, "torch", False, True), (1000, "torch", False, True),
                                                           (1000, "r3dgs", True, True), (1000, "torch", False, False),
                                                           (4099, "r3dgs_capturable", False, True),
                                                           (SCAN_SPAN + 1, "r3dgs", True, True)])
def test_relocate_equals_the_reference(P, kind, zero_relocated, moments):
    state = _state(P, seed=P + 1, moments=moments)
    uniforms = np.random.default_rng(P).random(P).astype(F32)
    pc, stats, worst, n = _relocate_and_check(state, kind, zero_relocated, uniforms)
    print(f"\nrelocate P={P} {kind}: {n} draws, worst error / bound = {worst:.3f}")
    if P >= 1000:
        assert n > P // 20 and int(stats["n_sources"]) > 10
    # two runs on the same inputs give the same bits
    pc2, stats2, _, _ = _relocate_and_check(state, kind, zero_relocated, uniforms)
    for attr in ATTRS.values():
        assert torch.equal(getattr(pc, attr).detach(), getattr(pc2, attr).detach()), attr
    assert all(torch.equal(stats[k], stats2[k]) for k in ("totals", "ratio")) and torch.equal(stats["sampled"][:n], stats2["sampled"][:n])


@pytest.mark.parametrize("P,kind,zero_relocated", [(64, "torch", False), (65, "r3dgs", True), (257, "torch", True)])
def test_relocate_at_the_wave_and_workgroup_edges_of_the_rank(P, kind, zero_relocated):
    """One full wave, one lane of a second wave, one lane of a second workgroup (csrc/block_scan.h block_rank): dead and drawn
    rows on both sides of every edge the model has, so that `slots` and the compacted cdf take ranks from across it."""
    state = _state(P, seed=P + 7)
    edges = [i for i in (0, 63, 64, 255, 256) if i < P]
    state["opacity"][edges] = -8.0                                    # dead
    state["opacity"][[i + 1 for i in edges if i + 1 < P and i + 1 not in edges]] = 1.5   # alive
    uniforms = np.random.default_rng(P).random(P).astype(F32)
    uniforms[0], uniforms[1] = 0.0, BELOW_ONE                         # the first and the last row of positive weight
    _, stats, worst, n = _relocate_and_check(state, kind, zero_relocated, uniforms)
    dead = ref.weights(state["opacity"].reshape(-1), MIN_OPACITY, ref.RELOCATE)[1]   # _check_plan held slots to flatnonzero(dead)
    assert dead[edges].all() and not dead[[i + 1 for i in edges if i + 1 < P and i + 1 not in edges]].any()
    assert int(stats["n_dead"]) == int(dead.sum()) == n >= len(edges)
    print(f"\nrelocate P={P} {kind}: {n} draws over the edges {edges}, worst error / bound = {worst:.3f}")


def test_sixty_with_fifty_nine_dead_clamps_the_ratio():
    state = _state(60, seed=3)
    state["opacity"][:] = -8.0
    state["opacity"][17] = 1.0
    _, stats, worst, n = _relocate_and_check(state, "torch", False, np.random.default_rng(1).random(60).astype(F32))
    assert n == 59 and stats["totals"].tolist() == [59, 59, 1, 1, 0, 1, 0, 0]
    assert int(stats["ratio"][17]) == 51 and torch.equal(stats["sampled"][:59], torch.full((59,), 17, dtype=torch.int32, device="cuda"))
    print(f"\nrelocate 60/59 dead: ratio 60 clamped to 51, worst error / bound = {worst:.3f}")


def test_special_inputs_of_the_plan():
    """Dead rows at index 0 and at P - 1 with u = 0 and u = the largest float below 1; raw opacities of +-20; all dead; none
    dead; an empty model."""
    import r3dgs_mcmc as mc
    P = 1000
    state = _state(P, seed=9)
    state["opacity"][0] = state["opacity"][-1] = -20.0
    state["opacity"][1:4] = -20.0
    state["opacity"][500:520] = 20.0
    state["opacity"][520:540] = -20.0
    uniforms = np.random.default_rng(2).random(P).astype(F32)
    uniforms[0], uniforms[1], uniforms[2], uniforms[3] = 0.0, BELOW_ONE, 0.0, BELOW_ONE
    bounded = ref.sigmoid64(state["opacity"].reshape(-1)) <= MAX_SIGMOID
    pc, stats, _, n = _relocate_and_check(state, "torch", False, uniforms, bounded)
    w, dead = ref.weights(state["opacity"].reshape(-1), MIN_OPACITY, ref.RELOCATE)
    alive = np.flatnonzero(~dead)
    sampled = stats["sampled"][:n].cpu().numpy()
    assert dead[0] and dead[-1] and sampled[0] == sampled[2] == alive[0] and sampled[1] == sampled[3] == alive[-1]
    assert all(torch.isfinite(getattr(pc, a)).all() for a in ATTRS.values())
    # all dead: nothing is alive, the plan is a no-op and says so
    for value, flag in ((-9.0, 1), (2.0, 2)):
        state = _state(333, seed=4)
        state["opacity"][:] = value
        pc, stats, _, n = _relocate_and_check(state, "r3dgs", True, uniforms[:333])
        assert n == 0 and int(stats["noop"]) == flag and int(stats["n_dead"]) == (333 if flag == 1 else 0)
        assert (stats["ratio"] == 1).all()
    # the empty model
    pc = _model(densify_ref.random_state(0, 4, seed=0))
    stats = mc.relocate(pc, MIN_OPACITY)
    assert stats["totals"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and pc._xyz.shape == (0, 3)
    mc.inject_noise(pc, 1.0)
    assert mc.add_new(pc, 100)["n_new"] == 0 and pc._xyz.shape == (0, 3)


@pytest.mark.parametrize("P,cap,kind,moments", [(1, 100, "torch", True), (60, 1000, "torch", True), (1000, 1020, "r3dgs", True),
                                                (1000, 5000, "torch", False), (4099, 10 ** 6, "r3dgs_capturable", True),
                                                (SCAN_SPAN + 1, 10 ** 6, "torch", True), (1000, 1000, "r3dgs", True)])
def test_add_new_equals_the_reference(P, cap, kind, moments):
    import r3dgs_mcmc as mc
    state = _state(P, seed=P + 2, moments=moments)
    n_new = ref.n_new(P, cap)
    uniforms = np.random.default_rng(P + 5).random(n_new).astype(F32)
    if n_new >= 2:
        uniforms[0], uniforms[1] = 0.0, BELOW_ONE
    pc = _model(state, kind)
    before = _snapshot(pc)
    stats = mc.add_new(pc, cap, uniforms=_dev(uniforms))
    assert stats["n_new"] == n_new == mc.n_new_rows(P, cap)
    if n_new == 0:   # the cap is reached (or 5 % of P is less than one row): nothing changes, no tensor object is replaced
        after = _snapshot(pc)
        assert all(after[k] is before[k] for k in before) and stats["totals"].tolist() == [0, 0, 0, 0, 2, 0, 0, 0]
        for name, attr in ATTRS.items():
            assert _same(getattr(pc, attr), state[name])
        return
    sampled, _, ratio = _check_plan(state["opacity"].reshape(-1), ref.GROW, uniforms, stats, n_new)
    assert len(sampled) == n_new
    out, upd = ref.grow(state, sampled, ratio, mc.GROW_MIN_OPACITY)
    rows = P + n_new
    for group in pc.optimizer.param_groups:   # the hand-over, as r3dgs_densify's
        p = group["params"][0]
        assert p is getattr(pc, ATTRS[group["name"]]) and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == rows
        if moments:
            assert pc.optimizer.state[p] is before[group["name"] + ".state"] and pc.optimizer.state[p]["step"] is before[group["name"] + ".step"]
            assert float(pc.optimizer.state[p]["step"]) == 7.0
    assert len(pc.optimizer.state) == (len(ATTRS) if moments else 0)
    for name, attr in ATTRS.items():
        if name not in ("opacity", "scaling"):
            assert _same(getattr(pc, attr), out[name]), name
        if moments:
            st = pc.optimizer.state[getattr(pc, attr)]
            assert _same(st["exp_avg"], out["exp_avg"][name]) and _same(st["exp_avg_sq"], out["exp_avg_sq"][name]), name
            assert not st["exp_avg"][P:].any() and not st["exp_avg_sq"][P:].any()
    assert _same(pc._degrees, out["degrees"])
    assert _same(pc.xyz_gradient_accum, np.zeros((rows, 1), F32)) and _same(pc.denom, np.zeros((rows, 1), F32))
    assert _same(pc.max_radii2D, np.zeros(rows, F32))
    worst = _check_updated(pc, state, out, upd, (np.arange(P, rows), sampled))
    print(f"\nadd_new P={P} -> {rows} {kind}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("P", [1, 1000, 4099])
def test_noise_equals_the_reference(P):
    import r3dgs_mcmc as mc
    state = _state(P, seed=P + 3)
    rng = np.random.default_rng(P)
    state["opacity"][:] = rng.normal(-5.5, 1.5, (P, 1)).astype(F32)   # around the gate's centre, sigmoid = 0.005
    state["opacity"][5:15] = 20.0
    state["opacity"][15:25] = -20.0
    noise = rng.standard_normal((P, 3)).astype(F32)
    noise[3::7] = 0
    state["xyz"][3::14] = -0.0
    scale = 5e5 * 1.6e-4
    want = ref.noise_delta(state["opacity"], state["scaling"], state["rotation"], noise, scale)
    runs = []
    for _ in range(2):
        pc = _model(state)
        before = _snapshot(pc)
        mc.inject_noise(pc, scale, noise=_dev(noise))
        assert pc._xyz is before["xyz"] and all(_same(getattr(pc, ATTRS[n]), state[n]) for n in ATTRS if n != "xyz")
        runs.append(pc._xyz.detach().cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), "not bit-identical from run to run"
    got = runs[0]
    assert np.array_equal(got[3::7].view(np.uint32), state["xyz"][3::7].view(np.uint32)), "a zero noise row leaves the bits of xyz"
    # the displacement itself, free of the rounding of the final add: the same call on xyz = 0
    zero = dict(state, xyz=np.zeros((P, 3), F32))
    pc = _model(zero)
    mc.inject_noise(pc, scale, noise=_dev(noise))
    delta = pc._xyz.detach().cpu().numpy().astype(np.float64)
    err, top = np.abs(delta - want), np.abs(want).max()
    print(f"\nnoise P={P}: max error / max|ref| = {err.max() / top:.3g}, worst per-element error / bar = "
          f"{(err / (1e-4 * np.abs(want) + 1e-6 * top)).max():.3g}")
    assert top > 0 and err.max() <= 1e-4 * top
    assert (err <= 1e-4 * np.abs(want) + 1e-6 * top).all()
    # and xyz_after - xyz_before is that displacement up to the rounding of the one add
    moved = got.astype(np.float64) - state["xyz"].astype(np.float64)
    assert (np.abs(moved - delta) <= 2.0 ** -24 * np.abs(got) + 1e-45).all()
    # drawn noise is seeded by the generator
    gen = torch.Generator(device="cuda").manual_seed(5)
    drawn = torch.randn((P, 3), generator=gen, device="cuda")
    a, b = _model(state), _model(state)
    mc.inject_noise(a, scale, noise=drawn)
    mc.inject_noise(b, scale, generator=gen.manual_seed(5))
    assert torch.equal(a._xyz.detach(), b._xyz.detach())


def test_noise_and_relocate_replay_from_a_graph_bit_for_bit():
    import r3dgs_mcmc as mc
    P = 4099
    state = _state(P, seed=77)
    noise = _dev(np.random.default_rng(1).standard_normal((P, 3)).astype(F32))
    uniforms = _dev(np.random.default_rng(2).random(P).astype(F32))
    eager, captured, warm = _model(state, "r3dgs"), _model(state, "r3dgs"), _model(state, "r3dgs")

    def run(pc):
        mc.inject_noise(pc, 80.0, noise=noise)
        return mc.relocate(pc, MIN_OPACITY, uniforms=uniforms, zero_relocated=True)
    want = run(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run(captured)
    graph.replay()
    torch.cuda.synchronize()
    assert int(want["n_draws"]) > 100 and torch.equal(got["totals"], want["totals"]) and torch.equal(got["ratio"], want["ratio"])
    for attr in ATTRS.values():
        a, b = getattr(eager, attr), getattr(captured, attr)
        assert torch.equal(a.detach(), b.detach()), attr
        sa, sb = eager.optimizer.state[a], captured.optimizer.state[b]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert torch.equal(eager._degrees, captured._degrees)


def test_two_hundred_steps_with_the_strategy_reach_the_cap():
    """A small training loop of our own with MCMCStrategy in place of densify_and_prune: 16 cameras, cap_max twice the start
    count.  The count never decreases and ends exactly at the cap, every tensor stays finite, the loss ends below its start."""
    import r3dgs_mcmc as mc
    import r3dgs_render
    W = H = 64
    P0 = 1500
    base = ss.make_camera(W, H, 60.0, None)
    g = ss.make_gaussians(P0, base, seed=41, degree_mode="mixed", scale_mu=0.05, zmin=2.0, zmax=8.0)
    cams = [_Cam(ss.make_camera(W, H, 60.0, k), W, H) for k in range(16)]
    bg = _dev(np.array([0.1, 0.2, 0.3], F32))
    state = {"xyz": g["means3D"], "f_dc": g["sh"][:, :1], "f_rest": g["sh"][:, 1:], "opacity": g["opacity"],
             "scaling": np.log(g["scales"]).astype(F32), "rotation": g["rotations"], "degrees": g["degrees"],
             "xyz_gradient_accum": np.zeros((P0, 1), F32), "denom": np.zeros((P0, 1), F32), "max_radii2D": np.zeros(P0, F32)}
    state = {k: np.ascontiguousarray(v) for k, v in state.items()}
    pc = _model(state, "r3dgs")
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3}
    for group in pc.optimizer.param_groups:
        group["lr"] = lrs[group["name"]]
    gen = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():
        targets = [r3dgs_render.render(c, pc, _Pipe, bg)["render"].clone() for c in cams]
        pc._xyz.add_(0.03 * torch.randn(pc._xyz.shape, device="cuda", generator=gen))
        pc._features_dc.mul_(0.5)
        pc._opacity[::10] = -7.0   # a tenth of the model starts dead
    strategy = mc.MCMCStrategy(cap_max=2 * P0, refine_start=5, refine_stop=200, refine_every=10, generator=gen)
    counts, losses = [P0], []
    for it in range(1, 201):
        k = it % len(cams)
        pc.optimizer.zero_grad(set_to_none=True)
        out = r3dgs_render.render(cams[k], pc, _Pipe, bg)
        l1 = (out["render"] - targets[k]).abs().mean()
        (l1 + mc.regularisation(pc)).backward()
        losses.append(l1.detach())
        pc.optimizer.step()
        stats = strategy.step_post_backward(pc, it, lrs["xyz"])
        assert (stats is not None) == (it % 10 == 0 and 5 < it < 200)
        counts.append(pc._xyz.shape[0])
    assert all(b >= a for a, b in zip(counts, counts[1:])), "the count decreased"
    assert counts[-1] == 2 * P0, counts[-1]
    for attr in ATTRS.values():
        p = getattr(pc, attr)
        assert torch.isfinite(p).all() and p.shape[0] == 2 * P0, attr
        st = pc.optimizer.state[p]
        assert torch.isfinite(st["exp_avg"]).all() and torch.isfinite(st["exp_avg_sq"]).all()
    losses = torch.stack(losses).cpu().numpy()
    first, last = float(losses[:16].mean()), float(losses[-16:].mean())
    print(f"\nMCMC loop: P {counts[0]} -> {counts[-1]} (reached at step {counts.index(2 * P0)}), L1 {first:.4f} -> {last:.4f}")
    assert np.isfinite(losses).all() and last < first
