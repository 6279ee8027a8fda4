"""CPU checks of the fused Adam step (reduced-3dgs_amd/r3dgs_optim.py, csrc/optim.hip, include/r3dgs_optim.h): the
per-element kernel arithmetic (csrc/adam_math.h) runs on the host through a test shim and must equal a numpy restatement
that rounds where the header documents, bit for bit; the Python surface keeps torch.optim.Adam's defaults and state keys,
refuses what the kernel does not implement, and its state_dict() loads into torch.optim.Adam and back.  No GPU needed."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import r3dgs_optim
from tests import adam_ref
from tests.hostcheck_build import EXACT, build_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck_optim", "hostcheck_optim.hip")
SO = os.path.join(HERE, "hostcheck_optim", "libhostcheck_optim.so")
F32 = np.float32


def _shim():
    return build_shim(SRC, SO, EXACT, "hipcc not available to build the optimizer host-check shim")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_step(lib, s, p, g, m, v):
    p, m, v = (np.array(x, F32) for x in (p, m, v))
    g = np.ascontiguousarray(g, F32)
    sc = np.array([s["w1"], s["beta2"], s["w2"], s["bc2_sqrt"], s["eps"], s["step_size"]], F32)
    lib.hc_adam_step(len(p), _p(sc), _p(g), _p(p), _p(m), _p(v))
    return p, m, v


def _inputs(rng, n, kind):
    p = (rng.standard_normal(n) * 3).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)).astype(F32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 2, n)).astype(F32)
    v = (10.0 ** rng.uniform(-30, 4, n)).astype(F32)
    if kind == "zeros":
        g[::3], m[1::3], v[2::3] = 0, 0, 0
        p[::7] = 0
    elif kind == "tiny_v":
        v = (10.0 ** rng.uniform(-45, -30, n)).astype(F32)
        g = (g * F32(1e-20)).astype(F32)
    elif kind == "huge_g":
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(15, 18, n)).astype(F32)
    return p, g, m, v


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def test_fma_emulation_is_exact():
    """The restatement's fma against exact rational arithmetic, including ties that a float64 sum rounds wrongly."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(2000) * 10.0 ** rng.uniform(-5, 5, 2000)).astype(F32)
    b = (rng.standard_normal(2000) * 10.0 ** rng.uniform(-5, 5, 2000)).astype(F32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.uniform(-1e-6, 1e-6, 2000))).astype(F32)
    # a * b + c = 1 + 2^-24 + 2^-60: float64 rounds the sum to the float32 tie 1 + 2^-24, which breaks to even (1.0)
    a = np.append(a, F32(1 + 2.0 ** -23)).astype(F32)
    b = np.append(b, F32(1 + 2.0 ** -23)).astype(F32)
    c = np.append(c, F32(-2.0 ** -23 - 2.0 ** -24)).astype(F32)
    got = adam_ref.fma32(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.float32(float(exact)), None
        # the correctly rounded float32 of `exact`: compare the two neighbours of float32(float(exact))
        cands = [np.nextafter(lo, F32(-np.inf)), lo, np.nextafter(lo, F32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - exact), int(np.asarray(q, F32).view(np.uint32)) & 1))
        assert np.asarray(r, F32).view(np.uint32) == np.asarray(best, F32).view(np.uint32), (x, y, z)


@pytest.mark.parametrize("kind", ["random", "zeros", "tiny_v", "huge_g"])
@pytest.mark.parametrize("step", [1, 2, 10_000])
@pytest.mark.parametrize("group", adam_ref.GROUPS, ids=[g[0] for g in adam_ref.GROUPS])
def test_header_on_host_matches_the_restatement_bit_for_bit(kind, step, group):
    """csrc/adam_math.h, run on the CPU, equals the float32 restatement (tests/adam_ref.step32) bit for bit -- p, m and v --
    with the reference's lrs, eps 1e-15 and torch's default betas."""
    lib = _shim()
    rng = np.random.default_rng(hash((kind, step, group[0])) % 2 ** 32)
    p, g, m, v = _inputs(rng, 20_000, kind)
    s = adam_ref.host_scalars(group[2], 0.9, 0.999, 1e-15, step)
    got = _host_step(lib, s, p, g, m, v)
    ref = adam_ref.step32(p, g, m, v, s)
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, ref):
        assert _bits_equal(a, b), f"{name}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements differ"


@pytest.mark.parametrize("betas,eps", [((0.3, 0.99), 1e-8), ((0.5, 0.5), 1e-6), ((0.0, 0.0), 1e-8)])
def test_header_other_betas(betas, eps):
    """The lerp's other form (1 - beta1 >= 0.5) and per-group betas / eps."""
    lib = _shim()
    rng = np.random.default_rng(11)
    p, g, m, v = _inputs(rng, 20_000, "random")
    s = adam_ref.host_scalars(0.01, betas[0], betas[1], eps, 7)
    got = _host_step(lib, s, p, g, m, v)
    ref = adam_ref.step32(p, g, m, v, s)
    for a, b in zip(got, ref):
        assert _bits_equal(a, b)


def test_restatement_is_close_to_float64():
    """Sanity of the restatement itself: one step in float32 is within a few ulp of float64 for ordinary values."""
    rng = np.random.default_rng(5)
    p, g, m, v = (rng.standard_normal(1000).astype(F32) for _ in range(4))
    v = np.abs(v)
    s = adam_ref.host_scalars(0.01, 0.9, 0.999, 1e-8, 3)
    p32, m32, v32 = adam_ref.step32(p, g, m, v, s)
    p64, m64, v64 = adam_ref.step64(p, g, m, v, 0.01, 0.9, 0.999, 1e-8, 3)
    assert np.abs(p32 - p64).max() <= 1e-5 * np.abs(p64 - p).max() + 1e-6
    assert np.allclose(m32, m64, rtol=1e-5, atol=1e-7) and np.allclose(v32, v64, rtol=1e-5, atol=1e-7)


def test_constructor_defaults_match_torch():
    mine = inspect.signature(r3dgs_optim.Adam.__init__).parameters
    theirs = inspect.signature(torch.optim.Adam.__init__).parameters
    for name in ("lr", "betas", "eps", "weight_decay", "amsgrad", "foreach", "maximize", "capturable", "differentiable",
                 "fused"):
        assert mine[name].default == theirs[name].default, name
    p = torch.nn.Parameter(torch.zeros(3))
    a, b = r3dgs_optim.Adam([p]), torch.optim.Adam([p])
    assert a.defaults == b.defaults
    a = r3dgs_optim.Adam([{"params": [p], "lr": 0.5, "betas": (0.8, 0.99), "eps": 1e-6}], lr=0.0, eps=1e-15)
    assert a.param_groups[0]["betas"] == (0.8, 0.99) and a.param_groups[0]["eps"] == 1e-6


@pytest.mark.parametrize("kw,match", [(dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"),
                                      (dict(weight_decay=0.01), "weight_decay"), (dict(differentiable=True), "differentiable"),
                                      (dict(foreach=True), "foreach"), (dict(foreach=False), "foreach"),
                                      (dict(fused=True), "fused"), (dict(lr=torch.tensor(0.01)), "Tensor lr")])
def test_refused_options(kw, match):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match=match):
        r3dgs_optim.Adam([p], **kw)
    with pytest.raises(ValueError, match=match):   # through a parameter group as well
        r3dgs_optim.Adam([{"params": [p], **kw}])


def _one(t, grad=None):
    p = torch.nn.Parameter(t)
    p.grad = torch.ones_like(t) if grad is None else grad
    return p


@pytest.mark.parametrize("make,match", [
    (lambda: _one(torch.zeros(4)), "host tensor"),
    (lambda: _one(torch.zeros(4, dtype=torch.float64)), "float32"),
    (lambda: _one(torch.zeros(4, dtype=torch.complex64)), "complex"),
    (lambda: _one(torch.zeros(4), torch.ones(4).to_sparse()), "sparse"),
])
def test_refused_tensors(make, match):
    opt = r3dgs_optim.Adam([make()])
    with pytest.raises(RuntimeError, match=match):
        opt.step()


def test_params_without_grad_get_no_state():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = r3dgs_optim.Adam([p])
    opt.step()
    assert len(opt.state) == 0


def _torch_state(p, steps, capturable=False):
    """A state as torch.optim.Adam leaves it after `steps` steps (values arbitrary)."""
    g = torch.Generator().manual_seed(steps)
    return {"step": torch.tensor(float(steps)) if not capturable else torch.tensor(float(steps), device=p.device),
            "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}


def _groups(n=20):
    params = [torch.nn.Parameter(torch.randn((n,) + shape)) for _, shape, _ in adam_ref.GROUPS]
    return params, [{"params": [p], "lr": lr, "name": name} for p, (name, _, lr) in zip(params, adam_ref.GROUPS)]


def test_state_dict_round_trips_with_torch():
    """state_dict() of torch.optim.Adam loads into r3dgs_optim.Adam and back, keys, dtypes and values unchanged; this is
    the reference's capture() / restore() path."""
    params, groups = _groups()
    theirs = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for i, p in enumerate(params):
        if i != 3:   # one parameter never had a gradient: no state
            theirs.state[p] = _torch_state(p, 7)
    sd = theirs.state_dict()
    params2, groups2 = _groups()
    mine = r3dgs_optim.Adam(groups2, lr=0.0, eps=1e-15)
    mine.load_state_dict(sd)
    sd2 = mine.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    assert sorted(sd2["state"]) == sorted(sd["state"]) and 3 not in sd2["state"]
    for k, st in sd["state"].items():
        assert set(sd2["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
        for key in st:
            a, b = sd2["state"][k][key], st[key]
            assert a.dtype == b.dtype == torch.float32 and a.device == b.device and torch.equal(a, b), (k, key)
    assert sd2["state"][0]["step"].device.type == "cpu" and sd2["state"][0]["step"].dim() == 0
    params3, groups3 = _groups()
    back = torch.optim.Adam(groups3, lr=0.0, eps=1e-15)
    back.load_state_dict(sd2)
    for p3, p in zip(params3, params):
        if p in theirs.state:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(back.state[p3][key], theirs.state[p][key])


def test_state_dict_keeps_group_names_and_lrs():
    """update_learning_rate finds groups by 'name' and writes 'lr': both survive the round trip."""
    params, groups = _groups()
    mine = r3dgs_optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in mine.param_groups:
        if g["name"] == "xyz":
            g["lr"] = 1.25e-4
    sd = mine.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == [g[0] for g in adam_ref.GROUPS]
    assert sd["param_groups"][0]["lr"] == 1.25e-4
    theirs = torch.optim.Adam(_groups()[1], lr=0.0, eps=1e-15)
    theirs.load_state_dict(sd)
    assert theirs.param_groups[0]["lr"] == 1.25e-4


def test_step_is_refused_inside_capture_without_capturable(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="capturable=True"):
        r3dgs_optim.Adam([p]).step()
