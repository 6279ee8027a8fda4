"""GPU checks of the fused Adam step (reduced-3dgs_amd/r3dgs_optim.py, csrc/optim.hip): bit-identical to torch.optim.Adam's
default (foreach) step on the reference's six groups, through densify / prune surgery, with missing gradients, odd sizes and
gradient views at odd offsets; deterministic and identical through both bindings; the capturable step against float64 and
torch's capturable step, graph capture against eager, and rasterizer training steps against torch.optim.Adam."""
import warnings

import numpy as np
import pytest
import torch

import r3dgs_optim
from diff_gaussian_rasterization import _C
from tests import adam_ref

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    diff = int((_bits(a) != _bits(b)).sum())
    assert diff == 0, f"{what}: {diff} of {a.numel()} elements differ"


def make_params(P, seed=0):
    """The reference's six leaves at P Gaussians, on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn((P,) + shape, device="cuda", generator=g) for _, shape, _ in adam_ref.GROUPS]


def make_opt(cls, tensors, **kw):
    params = [torch.nn.Parameter(t.clone()) for t in tensors]
    groups = [{"params": [p], "lr": lr, "name": name} for p, (name, _, lr) in zip(params, adam_ref.GROUPS)]
    return params, cls(groups, lr=0.0, eps=1e-15, **kw)


def update_learning_rate(opt, it):
    """As the reference's update_learning_rate: the xyz group's lr is rewritten every iteration."""
    for group in opt.param_groups:
        if group["name"] == "xyz":
            group["lr"] = adam_ref.xyz_lr(it)


def random_grads(params, gen):
    return [torch.randn(p.shape, device="cuda", generator=gen) * 10.0 ** torch.empty(p.shape, device="cuda").uniform_(
        -6, 1, generator=gen) for p in params]


def assert_same_state(mine, theirs, pm, pt, what):
    for i, (a, b) in enumerate(zip(pm, pt)):
        assert_same_bits(a, b, f"{what}: param {i}")
        sa, sb = mine.state[a], theirs.state[b]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        assert sa["step"].item() == sb["step"].item() and sa["step"].device == sb["step"].device
        assert_same_bits(sa["exp_avg"], sb["exp_avg"], f"{what}: exp_avg {i}")
        assert_same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"], f"{what}: exp_avg_sq {i}")


def prune_and_densify(opt, params, keep, n_new, gen):
    """A densify / prune stand-in: each group keeps the rows of `keep` and appends n_new rows copied from the first kept
    ones (the new rows get zero moments), on new nn.Parameters whose state is the old one masked and concatenated --
    what the reference's _prune_optimizer and cat_tensors_to_optimizer do to the optimizer."""
    out = []
    for group, p in zip(opt.param_groups, params):
        assert group["params"][0] is p
        st = opt.state.pop(p, None)
        kept = p.detach()[keep]
        new_rows = kept[:n_new] + 0.01 * torch.randn(kept[:n_new].shape, device="cuda", generator=gen)
        q = torch.nn.Parameter(torch.cat([kept, new_rows]).contiguous())
        if st is not None:
            z = torch.zeros_like(new_rows)
            st["exp_avg"] = torch.cat([st["exp_avg"][keep], z]).contiguous()
            st["exp_avg_sq"] = torch.cat([st["exp_avg_sq"][keep], z]).contiguous()
            opt.state[q] = st
        group["params"][0] = q
        out.append(q)
    return out


@pytest.mark.parametrize("P", [20_000, 500_000])
def test_bit_identical_to_torch_adam(P):
    """One step and 200 steps, random gradients, the xyz lr changing every step: params, exp_avg and exp_avg_sq equal
    torch.optim.Adam's (default foreach path) bit for bit."""
    init = make_params(P, seed=1)
    pm, mine = make_opt(r3dgs_optim.Adam, init)
    pt, theirs = make_opt(torch.optim.Adam, init)
    gen = torch.Generator(device="cuda").manual_seed(2)
    for it in range(1, 201):
        update_learning_rate(mine, it)
        update_learning_rate(theirs, it)
        for a, b, g in zip(pm, pt, random_grads(pm, gen)):
            a.grad, b.grad = g, g.clone()
        mine.step()
        theirs.step()
        mine.zero_grad(set_to_none=True)
        theirs.zero_grad(set_to_none=True)
        if it in (1, 200):
            assert_same_state(mine, theirs, pm, pt, f"P={P} step {it}")


def test_bit_identical_through_densify_and_prune():
    """Every 20 steps both optimizers go through the same prune + densify surgery; parity stays bit for bit."""
    P = 20_000
    init = make_params(P, seed=3)
    pm, mine = make_opt(r3dgs_optim.Adam, init)
    pt, theirs = make_opt(torch.optim.Adam, init)
    gen = torch.Generator(device="cuda").manual_seed(4)
    for it in range(1, 101):
        update_learning_rate(mine, it)
        update_learning_rate(theirs, it)
        for a, b, g in zip(pm, pt, random_grads(pm, gen)):
            a.grad, b.grad = g, g.clone()
        mine.step()
        theirs.step()
        mine.zero_grad(set_to_none=True)
        theirs.zero_grad(set_to_none=True)
        if it % 20 == 0:
            n = pm[0].shape[0]
            keep = torch.rand(n, device="cuda", generator=gen) > 0.15
            n_new = int(0.2 * int(keep.sum()))
            s = gen.get_state()
            pm = prune_and_densify(mine, pm, keep, n_new, gen)
            gen.set_state(s)
            pt = prune_and_densify(theirs, pt, keep, n_new, gen)
            assert pm[0].shape[0] != n
            assert_same_state(mine, theirs, pm, pt, f"after surgery at step {it}")
    assert_same_state(mine, theirs, pm, pt, "step 100")


def test_missing_grads_and_odd_sizes():
    """Tensors of 1, 3, 4, 5 and 1 000 003 elements (shapes that leave heads and tails around the 16-byte body) and a
    parameter view at an odd float offset; some get no gradient in some steps (no state, no step bump)."""
    sizes = [1, 3, 4, 5, 1_000_003, 37]
    gen = torch.Generator(device="cuda").manual_seed(5)
    init = [torch.randn(n, device="cuda", generator=gen) for n in sizes]

    def param(t, last):
        if not last:
            return torch.nn.Parameter(t.clone())
        buf = torch.zeros(t.numel() + 3, device="cuda")
        buf[1:1 + t.numel()] = t
        return torch.nn.Parameter(buf[1:1 + t.numel()])   # storage offset of one float

    pm = [param(t, i == len(init) - 1) for i, t in enumerate(init)]
    pt = [param(t, i == len(init) - 1) for i, t in enumerate(init)]
    assert pm[-1].storage_offset() == 1
    mine = r3dgs_optim.Adam(pm, lr=0.01)
    theirs = torch.optim.Adam(pt, lr=0.01)
    for it in range(12):
        for i, (a, b) in enumerate(zip(pm, pt)):
            if (it + i) % 3 == 0 or (i == 0 and it < 5):
                a.grad = b.grad = None
            else:
                g = torch.randn(a.shape, device="cuda", generator=gen)
                a.grad, b.grad = g, g.clone()
        mine.step()
        theirs.step()
    assert len(mine.state) == len(theirs.state)
    for i, (a, b) in enumerate(zip(pm, pt)):
        assert (a in mine.state) == (b in theirs.state)
        assert_same_bits(a, b, f"size {sizes[i]}")
        if a in mine.state:
            assert mine.state[a]["step"].item() == theirs.state[b]["step"].item()
            assert_same_bits(mine.state[a]["exp_avg"], theirs.state[b]["exp_avg"], f"exp_avg size {sizes[i]}")
            assert_same_bits(mine.state[a]["exp_avg_sq"], theirs.state[b]["exp_avg_sq"], f"exp_avg_sq size {sizes[i]}")


def test_more_tensors_than_one_launch_holds():
    """70 tensors (the segment table holds 32 per launch): three launches, still torch's bits; in capturable mode every
    tensor's device step is bumped exactly once per step."""
    gen = torch.Generator(device="cuda").manual_seed(14)
    init = [torch.randn(17 + 13 * i, device="cuda", generator=gen) for i in range(70)]
    pm = [torch.nn.Parameter(t.clone()) for t in init]
    pt = [torch.nn.Parameter(t.clone()) for t in init]
    pc = [torch.nn.Parameter(t.clone()) for t in init]
    mine, theirs = r3dgs_optim.Adam(pm, lr=0.01), torch.optim.Adam(pt, lr=0.01)
    capt = r3dgs_optim.Adam(pc, lr=0.01, capturable=True)
    for _ in range(3):
        for a, b, c in zip(pm, pt, pc):
            g = torch.randn(a.shape, device="cuda", generator=gen)
            a.grad, b.grad, c.grad = g, g.clone(), g.clone()
        mine.step()
        theirs.step()
        capt.step()
    assert_same_state(mine, theirs, pm, pt, "70 tensors")
    assert all(capt.state[c]["step"].item() == 3.0 for c in pc)


@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_gradient_views_at_odd_offsets(base):
    """Gradients as views into one flat buffer at float offsets of every 16-byte phase (as multiview.set_gradient_arena
    makes them): the segments whose pointers disagree in phase run the scalar path, the others the vector path."""
    P = 10_001
    init = make_params(P, seed=6)
    pm, mine = make_opt(r3dgs_optim.Adam, init)
    pt, theirs = make_opt(torch.optim.Adam, init)
    gen = torch.Generator(device="cuda").manual_seed(7)
    total = sum(p.numel() for p in pm)
    for it in range(1, 6):
        arena = torch.randn(total + 8 * len(pm), device="cuda", generator=gen)
        off = base
        for a, b in zip(pm, pt):
            a.grad = arena[off:off + a.numel()].view(a.shape)
            b.grad = a.grad.clone()
            off += a.numel() + 1   # the next view one float further along: every phase occurs
        mine.step()
        theirs.step()
    assert_same_state(mine, theirs, pm, pt, f"arena base {base}")


def _run(P, steps, binding=None):
    was = _C.set_binding(binding) if binding else None
    try:
        init = make_params(P, seed=8)
        pm, opt = make_opt(r3dgs_optim.Adam, init)
        gen = torch.Generator(device="cuda").manual_seed(9)
        for it in range(1, steps + 1):
            update_learning_rate(opt, it)
            for a, g in zip(pm, random_grads(pm, gen)):
                a.grad = g
            opt.step()
        return [p.detach().clone() for p in pm] + [opt.state[p][k].clone() for p in pm for k in ("exp_avg", "exp_avg_sq")]
    finally:
        if was:
            _C.set_binding(was)


def test_deterministic():
    a, b = _run(50_000, 5), _run(50_000, 5)
    for x, y in zip(a, b):
        assert_same_bits(x, y, "run to run")


def test_both_bindings_identical():
    a, b = _run(50_000, 5, "ctypes"), _run(50_000, 5, "torch")
    for x, y in zip(a, b):
        assert_same_bits(x, y, "ctypes vs torch binding")


def test_capturable_against_float64_and_torch():
    """capturable=True: device step bumped by the kernel, bias corrections from it.  After 50 steps each tensor's p_k - p_0
    agrees with a float64 restatement and with torch.optim.Adam(capturable=True) within 1e-5 max|p_k - p_0|.  The parameters
    start near 0 (|p_0| ~ 1e-6), so that the rounding of p itself, which any fp32 optimizer performs each step, stays far
    below that bar and the comparison measures the update arithmetic."""
    P = 20_000
    init = [t * 1e-6 for t in make_params(P, seed=10)]
    pm, mine = make_opt(r3dgs_optim.Adam, init, capturable=True)
    pt, theirs = make_opt(torch.optim.Adam, init, capturable=True)
    p64 = [t.double().cpu().numpy() for t in init]
    m64 = [np.zeros_like(x) for x in p64]
    v64 = [np.zeros_like(x) for x in p64]
    gen = torch.Generator(device="cuda").manual_seed(11)
    for it in range(1, 51):
        update_learning_rate(mine, it)
        update_learning_rate(theirs, it)
        grads = random_grads(pm, gen)
        for i, (a, b, g) in enumerate(zip(pm, pt, grads)):
            a.grad, b.grad = g, g.clone()
            lr = adam_ref.xyz_lr(it) if i == 0 else adam_ref.GROUPS[i][2]
            p64[i], m64[i], v64[i] = adam_ref.step64(p64[i], g.double().cpu().numpy(), m64[i], v64[i], lr, 0.9, 0.999,
                                                     1e-15, it)
        mine.step()
        theirs.step()
    for i, (a, b) in enumerate(zip(pm, pt)):
        st = mine.state[a]["step"]
        assert st.is_cuda and st.dtype == torch.float32 and st.item() == 50.0
        d = (a.detach() - init[i]).double().cpu().numpy()
        d64 = p64[i] - init[i].double().cpu().numpy()
        dt = (b.detach() - init[i]).double().cpu().numpy()
        scale = np.abs(d64).max()
        assert np.abs(d - d64).max() <= 1e-5 * scale, f"group {i}: vs float64"
        assert np.abs(d - dt).max() <= 1e-5 * scale, f"group {i}: vs torch capturable"


def test_graph_capture_equals_eager():
    """A torch.cuda.graph capture of the capturable step, replayed with the device lr changed between replays, equals the
    same steps run eagerly bit for bit; a non-capturable step inside a capture is refused."""
    P = 20_000
    init = make_params(P, seed=12)
    lr_g = torch.tensor(1e-3, device="cuda")
    lr_e = torch.tensor(1e-3, device="cuda")
    pg = [torch.nn.Parameter(t.clone()) for t in init]
    pe = [torch.nn.Parameter(t.clone()) for t in init]
    og = r3dgs_optim.Adam(pg, lr=lr_g, capturable=True)
    oe = r3dgs_optim.Adam(pe, lr=lr_e, capturable=True)
    gen = torch.Generator(device="cuda").manual_seed(13)
    static_grads = [torch.zeros_like(p) for p in pg]
    for p, g in zip(pg, static_grads):
        p.grad = g
    # warm-up step outside the capture (lazy state), on a side stream as torch.cuda.graph expects
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        og.step()
    torch.cuda.current_stream().wait_stream(s)
    for p, g in zip(pe, static_grads):
        p.grad = g.clone()
    oe.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        og.step()
    for it in range(6):
        lr = 1e-3 * (0.7 ** it)
        lr_g.fill_(lr)
        lr_e.fill_(lr)
        grads = random_grads(pg, gen)
        for sg, g, p in zip(static_grads, grads, pe):
            sg.copy_(g)
            p.grad = g
        graph.replay()
        oe.step()
    torch.cuda.synchronize()
    for a, b in zip(pg, pe):
        assert_same_bits(a, b, "graph vs eager")
        assert og.state[a]["step"].item() == oe.state[b]["step"].item() == 7.0
        assert_same_bits(og.state[a]["exp_avg"], oe.state[b]["exp_avg"], "graph vs eager exp_avg")
        assert_same_bits(og.state[a]["exp_avg_sq"], oe.state[b]["exp_avg_sq"], "graph vs eager exp_avg_sq")
    plain = r3dgs_optim.Adam([torch.nn.Parameter(init[0].clone())], lr=1e-3)
    plain.param_groups[0]["params"][0].grad = torch.ones_like(init[0])
    plain.step()
    g2 = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():   # the refused step leaves the capture empty, which torch warns about
        warnings.simplefilter("ignore", UserWarning)
        with pytest.raises(RuntimeError, match="capturable=True"):
            with torch.cuda.graph(g2):
                plain.step()


def test_training_steps_match_torch_adam():
    """Rasterizer render + r3dgs_loss.l1_dssim + backward + step: with r3dgs_optim.Adam the parameters equal those of
    torch.optim.Adam bit for bit after each step.  Both optimizers take the same gradient each step (the parameters being
    equal, one render serves both)."""
    import diff_gaussian_rasterization as dgr
    import r3dgs_loss
    import synth_scene as ss
    w, cam, g = ss.make_workload("cfg0_10k_400", seed=0)
    W, H = w["W"], w["H"]

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    degrees = dv(g["degrees"])
    empty = torch.Tensor([])
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dv(np.zeros(3, np.float32)), 1.0,
                                           dv(cam.world_view_transform), dv(cam.full_proj_transform), 3,
                                           dv(cam.camera_center), False, False)
    gt = dv(np.random.default_rng(3).random((3, H, W)).astype(np.float32))
    names = ("means3D", "opacity", "scales", "rotations", "sh")
    lrs = (0.00016, 0.05, 0.005, 0.001, 0.0025)
    pm = [torch.nn.Parameter(dv(g[k])) for k in names]
    pt = [torch.nn.Parameter(dv(g[k])) for k in names]
    mine = r3dgs_optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(pm, lrs)], lr=0.0, eps=1e-15)
    theirs = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(pt, lrs)], lr=0.0, eps=1e-15)
    for it in range(5):
        leaves = dict(zip(names, pm))
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
        color, _ = dgr.rasterize_gaussians(leaves["means3D"], means2D, leaves["sh"], degrees, empty, leaves["opacity"],
                                           leaves["scales"], leaves["rotations"], empty, rs, 0.0)
        loss = r3dgs_loss.l1_dssim(color, gt, 0.2)[0]
        loss.backward()
        for a, b in zip(pm, pt):
            assert a.grad is not None and a.grad.abs().max() > 0
            b.grad = a.grad.clone()
        mine.step()
        theirs.step()
        mine.zero_grad(set_to_none=True)
        theirs.zero_grad(set_to_none=True)
        for k, a, b in zip(names, pm, pt):
            assert_same_bits(a, b, f"{k} after training step {it + 1}")
