"""GPU checks of the visibility-gated Adam step (r3dgs_optim.Adam.step(radii=...), csrc/optim.hip's adam_visible_kernel):
on the reference's six groups carved out of one flat buffer at every 16-byte phase, between sentinel guards, a gated step
equals the float32 restatement (tests/adam_ref.step32) and the dense step on the visible rows bit for bit, keeps the bits
of the others although their gradients hold NaN and Inf, equals the dense step over whole tensors when every row is
visible (plain and capturable), is identical through both bindings and bumps every count by one; twenty steps with a new
mask each equal the per-row restatement; a captured graph follows the contents of its radii buffer; checkpoints load into
torch.optim.Adam and back."""
import io

import numpy as np
import pytest
import torch

import r3dgs_optim
from diff_gaussian_rasterization import _C
from tests import adam_ref

pytestmark = pytest.mark.gpu

GUARD = 64                  # sentinel floats before and after every view
SENTINEL = 0x7fc5a5a5       # a quiet NaN with a payload: any arithmetic on it or any overwrite shows in the bits
SIZES = [0, 1, 2, 91, 92, 200, 1031]
# which layout each group gets is rotated per size, so that f_rest (the tensor of more than one chunk: 4095 and 4140 floats
# at 91 and 92 lie either side of one chunk of 1024 float4 units) meets vector heads and the scalar path
ROTATION = {0: 0, 1: 1, 2: 2, 91: 0, 92: 1, 200: 3, 1031: 2}
MASKS = ["all", "none", "alternating", "row0", "last", "runs16", "random30", "values"]
CAPTURABLE_RTOL = 1e-5      # tests/test_optim_gpu.py::test_capturable_against_float64_and_torch's bar on p_k - p_0
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _phases(kind):
    """Float offsets mod 4 of p, g, m, v.  kind 0-3: one shared phase (a vector row with head (4 - kind) % 4); 4 and 5:
    phases that disagree (a scalar row)."""
    return {4: (0, 1, 2, 3), 5: (2, 2, 1, 2)}.get(kind, (kind,) * 4)


class Arena:
    """The six groups' p, g, m, v as views into one flat buffer, each at a chosen 16-byte phase between two guards."""

    def __init__(self, P, rotation, seed, near_zero=False):
        self.P = P
        gen = torch.Generator(device="cuda").manual_seed(seed)
        spans, off = [], 0
        for i, (_, shape, _) in enumerate(adam_ref.GROUPS):
            n = P * int(np.prod(shape))
            for phase in _phases((i + rotation) % 6):
                off += GUARD
                off += (phase - off) % 4
                spans.append((off, n))
                off += n + GUARD
        self.buf = torch.full((off + 4,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0
        views = [self.buf[o:o + n] for o, n in spans]
        self.p, self.g, self.m, self.v = ([views[4 * i + j].view((P,) + adam_ref.GROUPS[i][1]) for i in range(6)]
                                          for j in range(4))
        self.written = torch.zeros(off + 4, dtype=torch.bool, device="cuda")   # what a step may write: p, m, v
        for k, (o, n) in enumerate(spans):
            if k % 4 != 1:
                self.written[o:o + n] = True
        for p, g, m, v in zip(self.p, self.g, self.m, self.v):
            p.copy_(torch.randn(p.shape, device="cuda", generator=gen) * (1e-6 if near_zero else 1.0))
            g.copy_(torch.randn(g.shape, device="cuda", generator=gen) *
                    10.0 ** torch.empty(g.shape, device="cuda").uniform_(-6, 1, generator=gen))
            m.copy_(torch.randn(m.shape, device="cuda", generator=gen) * 1e-2)
            v.copy_(torch.rand(v.shape, device="cuda", generator=gen) * 1e-3)
        for i in range(6):
            want = _phases((i + rotation) % 6)
            got = tuple((t.data_ptr() // 4) % 4 for t in (self.p[i], self.g[i], self.m[i], self.v[i]))
            assert P == 0 or got == want

    def clone(self):
        other = object.__new__(Arena)
        other.P, other.written = self.P, self.written
        other.buf = self.buf.clone()
        shift = lambda t: other.buf[t.storage_offset():t.storage_offset() + t.numel()].view(t.shape)   # noqa: E731
        other.p, other.g, other.m, other.v = ([shift(t) for t in ts] for ts in (self.p, self.g, self.m, self.v))
        return other

    def poison_invisible_gradients(self, vis):
        """NaN, +Inf and -Inf over the gradient rows of the invisible Gaussians."""
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda")
        for g in self.g:
            pattern = bad[torch.arange(g.numel(), device="cuda") % 3].view(g.shape)
            g.copy_(torch.where(vis.view((-1,) + (1,) * (g.dim() - 1)), g, pattern))

    def optimizer(self, step=None, **kw):
        """r3dgs_optim.Adam over the views; step: a state at that count on m and v (None: lazy state, m and v unused)."""
        params = [torch.nn.Parameter(p) for p in self.p]
        for q, p, g in zip(params, self.p, self.g):
            assert q.data_ptr() == p.data_ptr()
            q.grad = g
        opt = r3dgs_optim.Adam([{"params": [q], "lr": lr, "name": name} for q, (name, _, lr) in zip(params, adam_ref.GROUPS)],
                               lr=0.0, eps=1e-15, **kw)
        if step is not None:
            for q, m, v in zip(params, self.m, self.v):
                count = torch.tensor(float(step), device="cuda") if kw.get("capturable") else torch.tensor(float(step))
                opt.state[q] = {"step": count, "exp_avg": m, "exp_avg_sq": v}
        return params, opt

    def assert_guards(self, before, what):
        """Every float a step may not write -- the guards, the gaps and the gradients -- has the bits of `before`."""
        a, b = self.buf.view(torch.int32)[~self.written], before.buf.view(torch.int32)[~self.written]
        assert torch.equal(a, b), f"{what}: {int((a != b).sum())} floats outside p, m, v changed"


def make_radii(P, mask, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(1000 + seed)
    idx = torch.arange(P, device="cuda")
    if mask == "values":   # zero, negative and large positive values: visible iff > 0
        pool = torch.tensor([0, -5, I32_MIN, I32_MAX, 1, 2 ** 30, -1, 7], dtype=torch.int32, device="cuda")
        return pool[torch.randint(0, len(pool), (P,), device="cuda", generator=gen)].contiguous()
    vis = {"all": idx >= 0, "none": idx < 0, "alternating": idx % 2 == 0, "row0": idx == 0, "last": idx == P - 1,
           "runs16": (idx // 16) % 2 == 0, "random30": torch.rand(P, device="cuda", generator=gen) < 0.3}[mask]
    return torch.where(vis, 1 + idx % 40, -(idx % 3)).to(torch.int32).contiguous()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    diff = int((bits(a) != bits(b)).sum())
    assert diff == 0, f"{what}: {diff} of {a.numel()} elements differ"


def step32_of(arena, i, lr, step):
    s = adam_ref.host_scalars(lr, 0.9, 0.999, 1e-15, step)
    with np.errstate(all="ignore"):
        return adam_ref.step32(*(t[i].cpu().numpy() for t in (arena.p, arena.g, arena.m, arena.v)), s)


def dense_scalars(lr, step):
    s = adam_ref.host_scalars(lr, 0.9, 0.999, 1e-15, step)
    return [float(s[k]) for k in ("w1", "beta2", "w2", "bc2_sqrt", "eps", "step_size")]


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("P", SIZES)
def test_one_gated_step(P, mask):
    radii = make_radii(P, mask, seed=P)
    vis = radii > 0
    start = Arena(P, ROTATION[P], seed=P)
    start.poison_invisible_gradients(vis)
    results = {}
    for binding in ("ctypes", "torch"):
        was = _C.set_binding(binding)
        try:
            a = start.clone()
            params, opt = a.optimizer(step=3)
            opt.step(radii=radii)
            torch.cuda.synchronize()
        finally:
            _C.set_binding(was)
        a.assert_guards(start, f"{binding} binding")
        assert all(opt.state[q]["step"].item() == 4.0 and not opt.state[q]["step"].is_cuda for q in params)
        results[binding] = a
    a = results["ctypes"]
    assert torch.equal(a.buf.view(torch.int32), results["torch"].buf.view(torch.int32)), "the two bindings differ"
    dense = start.clone()   # the dense call on copies of the same inputs, NaN rows and all
    scalars = [x for _, _, lr in adam_ref.GROUPS for x in dense_scalars(lr, 4)]
    _C.adam_step(dense.p, dense.g, dense.m, dense.v, scalars)
    torch.cuda.synchronize()
    for i, (name, _, lr) in enumerate(adam_ref.GROUPS):
        ref = step32_of(start, i, lr, 4)
        for what, got, old, r, d in zip(("param", "exp_avg", "exp_avg_sq"), (a.p[i], a.m[i], a.v[i]),
                                        (start.p[i], start.m[i], start.v[i]), ref, (dense.p[i], dense.m[i], dense.v[i])):
            r = torch.from_numpy(r).cuda()
            assert_same_bits(got[vis], r[vis], f"{name} {what}: visible rows vs step32")
            assert_same_bits(got[vis], d[vis], f"{name} {what}: visible rows vs the dense step")
            assert_same_bits(got[~vis], old[~vis], f"{name} {what}: invisible rows")
            if mask == "all":
                assert_same_bits(got, d, f"{name} {what}: all visible vs the dense step")
    if mask == "all":   # whole buffers: nothing else differs either
        assert torch.equal(a.buf.view(torch.int32), dense.buf.view(torch.int32))


@pytest.mark.parametrize("P", SIZES)
def test_all_visible_equals_dense_capturable(P):
    """capturable=True, every row visible: the gated step equals the dense capturable step over whole buffers bit for bit,
    with a device lr, and both bump the device counts by one."""
    start = Arena(P, ROTATION[P], seed=100 + P)
    radii = make_radii(P, "all")
    lr = torch.tensor(3e-3, device="cuda")
    out = []
    for gated in (True, False):
        a = start.clone()
        params, opt = a.optimizer(step=5, capturable=True)
        opt.param_groups[0]["lr"] = lr
        if gated:
            opt.step(radii=radii)
        else:
            opt.step()
        torch.cuda.synchronize()
        assert all(opt.state[q]["step"].item() == 6.0 and opt.state[q]["step"].is_cuda for q in params)
        a.assert_guards(start, "capturable")
        out.append(a)
    assert torch.equal(out[0].buf.view(torch.int32), out[1].buf.view(torch.int32))
    if P:
        assert not torch.equal(out[0].buf.view(torch.int32), start.buf.view(torch.int32))


def test_capturable_gated_step_keeps_invisible_rows_and_bumps():
    """capturable=True under a mask, eagerly: invisible rows (NaN gradients) keep their bits, visible rows equal the dense
    capturable step, the counts advance by one; and with no Gaussians at all the counts still advance."""
    P = 92
    radii = make_radii(P, "random30", seed=5)
    vis = radii > 0
    start = Arena(P, 1, seed=77)
    start.poison_invisible_gradients(vis)
    a, dense = start.clone(), start.clone()
    params, opt = a.optimizer(step=2, capturable=True)
    opt.step(radii=radii)
    dparams, dopt = dense.optimizer(step=2, capturable=True)
    dopt.step()
    torch.cuda.synchronize()
    a.assert_guards(start, "capturable gated")
    for i in range(6):
        for got, old, d in zip((a.p[i], a.m[i], a.v[i]), (start.p[i], start.m[i], start.v[i]),
                               (dense.p[i], dense.m[i], dense.v[i])):
            assert_same_bits(got[vis], d[vis], f"group {i}: visible rows vs dense capturable")
            assert_same_bits(got[~vis], old[~vis], f"group {i}: invisible rows")
    assert all(opt.state[q]["step"].item() == 3.0 for q in params)
    empty = Arena(0, 0, seed=1)
    eparams, eopt = empty.optimizer(step=2, capturable=True)
    eopt.step(radii=make_radii(0, "all"))
    torch.cuda.synchronize()
    assert all(eopt.state[q]["step"].item() == 3.0 for q in eparams)


def test_twenty_steps_with_a_new_mask_each():
    """P = 200 (f_rest: three chunks of float4 units), a new random mask and xyz lr every step, lazily made state: the end
    state equals the per-row restatement -- the tensor's step count applied to the visible rows only -- bit for bit; rows
    never visible keep their initial parameter bits and all-zero moments."""
    P = 200
    a = Arena(P, 0, seed=21)
    start = a.clone()
    params, opt = a.optimizer()
    ref_p = [t.cpu().numpy().copy() for t in a.p]
    ref_m = [np.zeros_like(x) for x in ref_p]
    ref_v = [np.zeros_like(x) for x in ref_p]
    gen = torch.Generator(device="cuda").manual_seed(22)
    ever = torch.zeros(P, dtype=torch.bool, device="cuda")
    for it in range(1, 21):
        vis = (torch.rand(P, device="cuda", generator=gen) < 0.4) & (torch.arange(P, device="cuda") % 10 != 3)
        radii = torch.where(vis, 5, 0).to(torch.int32)
        ever |= vis
        opt.param_groups[0]["lr"] = adam_ref.xyz_lr(it)
        for g in a.g:
            g.copy_(torch.randn(g.shape, device="cuda", generator=gen) * 1e-2)
        a.poison_invisible_gradients(vis)
        opt.step(radii=radii)
        vis_h = vis.cpu().numpy()
        for i, (_, shape, lr) in enumerate(adam_ref.GROUPS):
            s = adam_ref.host_scalars(adam_ref.xyz_lr(it) if i == 0 else lr, 0.9, 0.999, 1e-15, it)
            g = np.where(vis_h.reshape((P,) + (1,) * len(shape)), a.g[i].cpu().numpy(), np.float32(0))
            p1, m1, v1 = adam_ref.step32(ref_p[i], g, ref_m[i], ref_v[i], s)
            sel = vis_h.reshape((P,) + (1,) * len(shape))
            ref_p[i], ref_m[i], ref_v[i] = (np.where(sel, new, old) for new, old in
                                            ((p1, ref_p[i]), (m1, ref_m[i]), (v1, ref_v[i])))
    torch.cuda.synchronize()
    assert 0 < int((~ever).sum()) < P
    for i, q in enumerate(params):
        st = opt.state[q]
        assert st["step"].item() == 20.0
        for what, got, ref in (("param", q, ref_p[i]), ("exp_avg", st["exp_avg"], ref_m[i]),
                               ("exp_avg_sq", st["exp_avg_sq"], ref_v[i])):
            assert_same_bits(got, torch.from_numpy(np.ascontiguousarray(ref)).cuda(), f"group {i} {what} after 20 steps")
        assert_same_bits(q[~ever], start.p[i][~ever], f"group {i}: rows never visible")
        assert not st["exp_avg"][~ever].any() and not st["exp_avg_sq"][~ever].any()


def test_captured_graph_follows_the_radii_buffer():
    """One capturable gated step captured on one stream with a fixed radii buffer and a device lr, replayed three times with
    new radii copied into the buffer: invisible rows keep their bits on each replay, the visible rows' p_k - p_0 agree with
    the float64 per-row restatement at the capturable step's bar, and the counts read 3."""
    P = 200
    warm = Arena(8, 0, seed=30)   # library and allocator warm-up on other tensors, on a side stream as torch.cuda.graph expects
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    warm_params, warm_opt = warm.optimizer(step=0, capturable=True)
    with torch.cuda.stream(side):
        warm_opt.step(radii=make_radii(8, "alternating"))
    torch.cuda.current_stream().wait_stream(side)
    a = Arena(P, 0, seed=31, near_zero=True)
    for m, v in zip(a.m, a.v):
        m.zero_()
        v.zero_()
    start = a.clone()
    lr = torch.tensor(1e-3, device="cuda")
    params, opt = a.optimizer(step=0, capturable=True)
    for group in opt.param_groups:
        group["lr"] = lr
    radii = torch.zeros(P, dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(radii=radii)
    torch.cuda.synchronize()
    assert torch.equal(a.buf.view(torch.int32), start.buf.view(torch.int32)), "the capture itself ran a step"
    p64 = [t.double().cpu().numpy() for t in start.p]
    m64 = [np.zeros_like(x) for x in p64]
    v64 = [np.zeros_like(x) for x in p64]
    gen = torch.Generator(device="cuda").manual_seed(32)
    for it, mask in enumerate(("random30", "runs16", "alternating"), start=1):
        new = make_radii(P, mask, seed=it)
        vis = new > 0
        radii.copy_(new)
        lr.fill_(1e-3 * 0.7 ** it)
        for g in a.g:
            g.copy_(torch.randn(g.shape, device="cuda", generator=gen) * 1e-2)
        a.poison_invisible_gradients(vis)
        before = a.clone()
        graph.replay()
        torch.cuda.synchronize()
        a.assert_guards(before, f"replay {it}")
        vis_h = vis.cpu().numpy()
        for i, (_, shape, _) in enumerate(adam_ref.GROUPS):
            for got, old in zip((a.p[i], a.m[i], a.v[i]), (before.p[i], before.m[i], before.v[i])):
                assert_same_bits(got[~vis], old[~vis], f"replay {it} group {i}: invisible rows")
            assert not torch.equal(bits(a.p[i][vis]), bits(before.p[i][vis])), f"replay {it} group {i}: nothing moved"
            sel = vis_h.reshape((P,) + (1,) * len(shape))
            g = np.where(sel, a.g[i].double().cpu().numpy(), 0.0)
            new64 = adam_ref.step64(p64[i], g, m64[i], v64[i], 1e-3 * 0.7 ** it, 0.9, 0.999, 1e-15, it)
            p64[i], m64[i], v64[i] = (np.where(sel, n, o) for n, o in zip(new64, (p64[i], m64[i], v64[i])))
    for i, q in enumerate(params):
        assert opt.state[q]["step"].item() == 3.0
        p0 = start.p[i].double().cpu().numpy()
        d = (a.p[i] - start.p[i]).double().cpu().numpy()
        d64 = p64[i] - p0
        assert np.abs(d - d64).max() <= CAPTURABLE_RTOL * np.abs(d64).max(), f"group {i}: vs float64"


def test_checkpoint_after_gated_steps_loads_into_torch_adam_and_back():
    P = 91
    a = Arena(P, 0, seed=40)
    params, opt = a.optimizer()
    for it in range(2):
        opt.step(radii=make_radii(P, "random30", seed=it))
    # a written checkpoint: state_dict() hands out the live state tensors and load_state_dict() keeps what it is given, so
    # without the file every optimizer below would count and accumulate in the same storage
    blob = io.BytesIO()
    torch.save(opt.state_dict(), blob)

    def checkpoint():
        blob.seek(0)
        return torch.load(blob, weights_only=True)

    def fresh(cls):
        ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
        return ps, cls([{"params": [q], "lr": lr, "name": name} for q, (name, _, lr) in zip(ps, adam_ref.GROUPS)],
                       lr=0.0, eps=1e-15)

    pt, theirs = fresh(torch.optim.Adam)
    theirs.load_state_dict(checkpoint())
    for q, t in zip(params, pt):
        assert set(theirs.state[t]) == {"step", "exp_avg", "exp_avg_sq"}
        assert theirs.state[t]["step"].item() == 2.0 and not theirs.state[t]["step"].is_cuda
        assert_same_bits(theirs.state[t]["exp_avg"], opt.state[q]["exp_avg"], "exp_avg into torch")
        assert_same_bits(theirs.state[t]["exp_avg_sq"], opt.state[q]["exp_avg_sq"], "exp_avg_sq into torch")
    for t in pt:
        t.grad = torch.ones_like(t)
    theirs.step()   # torch accepts the state as its own
    pb, back = fresh(r3dgs_optim.Adam)
    back.load_state_dict(checkpoint())
    radii = make_radii(P, "runs16")
    for q, b in zip(params, pb):
        b.grad = q.grad.clone()
    opt.step(radii=radii)
    back.step(radii=radii)
    for q, b in zip(params, pb):
        assert back.state[b]["step"].item() == opt.state[q]["step"].item() == 3.0
        assert_same_bits(b, q, "param after reload")
        assert_same_bits(back.state[b]["exp_avg"], opt.state[q]["exp_avg"], "exp_avg after reload")
        assert_same_bits(back.state[b]["exp_avg_sq"], opt.state[q]["exp_avg_sq"], "exp_avg_sq after reload")
