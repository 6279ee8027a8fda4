"""GPU tests (-m gpu) of the per-iteration training statistics (reduced-3dgs_amd/r3dgs_train_stats.py, csrc/train_stats.hip).

Shapes: P in {1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5} (one lane, the wave and workgroup edges, several partials to combine)
with M in {1, 2, 16} (no rest row, one coefficient, full rows), each with no Gaussian visible, all visible and a seeded ~40 %.
References: tests/trainstats_ref.py (numpy, float64 sums, float32 roundings where the kernel rounds) and the reference's own
torch lines run on the same device tensors.  Bars:
  * accumulators against the restatement: bit for bit;
  * against the torch lines: denom and max_radii2D exact; xyz_gradient_accum within 2 float32 ulp of the increment plus half
    an ulp of the sum -- torch's norm may contract its second square into an fma (<= 2 ulp of the increment between the two
    norms), and the kernel's one add rounds by at most half an ulp of its result.  So the kernel's accumulator is compared
    with old + torch's norm evaluated in float64: two float32 sums of increments that differ would otherwise be compared
    through two roundings;
  * n_visible and the mask exact; sh_abs_mean within 1 float32 ulp of the float64 mean (exact terms, double sum: only the final
    rounding); alpha_mean within trainstats_ref.SIGMOID_REL (4 U, every term is positive so the sum inherits the terms' relative
    bound) plus 1 ulp for the final rounding;
  * opacity.grad after (lambda * alpha_mean).backward(): old + increment in float64, within trainstats_ref.ALPHA_TERM_REL (the
    derivative's 6 U and the one multiply by upstream / n: 7 U) of the increment, plus half an ulp of the result for the
    accumulation into the pre-filled gradient, which is a float32 add the test cannot look inside.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import r3dgs_train_stats as ts
import synth_scene as ss
from tests import trainstats_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
PS = (1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5)
MS = (1, 2, 16)
PATTERNS = ("none", "all", "mix")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, F32))).astype(np.float64)


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _case(P, M, pattern, salt=0):
    """Host inputs of one shape; computed once and shared (never written to)."""
    rng = np.random.default_rng(zlib.crc32(f"{P}/{M}/{pattern}/{salt}".encode()))
    r = rng.integers(1, 300, P).astype(np.int32)
    if pattern == "none":
        radii = np.zeros(P, np.int32)
    elif pattern == "all":
        radii = r
    else:
        radii = np.where(rng.random(P) < 0.4, r, 0).astype(np.int32)
    c = dict(radii=radii,
             opacity=(rng.standard_normal((P, 1)) * 3).astype(F32),
             rest=(rng.standard_normal((P, M - 1, 3)) * 10.0 ** rng.uniform(-3, 0, (P, M - 1, 3))).astype(F32),
             vg=(rng.standard_normal((P, 3)) * 10.0 ** rng.uniform(-8, 3, (P, 3))).astype(F32),   # non-zero under culled rows too
             acc=(10.0 ** rng.uniform(-6, 2, (P, 1))).astype(F32),
             den=rng.integers(1, 3000, (P, 1)).astype(F32),
             mx=rng.choice(np.array([0.5, 1.0, 37.0, 150.0, 1000.0], F32), P).astype(F32),
             grad0=(rng.standard_normal((P, 1)) * 10.0 ** rng.uniform(-6, 0, (P, 1))).astype(F32))
    for v in c.values():
        v.setflags(write=False)
    return c


def _run_densification(c, vg=None):
    acc, den, mx = _dev(c["acc"]), _dev(c["den"]), _dev(c["mx"])
    ts.densification_stats(_dev(c["vg"]) if vg is None else vg, _dev(c["radii"]), acc, den, mx)
    return acc, den, mx


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", PS)
def test_densification_stats_equals_the_restatement_bit_for_bit(P, pattern):
    c = _case(P, 16, pattern)
    got = _run_densification(c)
    want = ref.densification_stats(c["vg"], c["radii"], c["acc"], c["den"], c["mx"])
    for name, a, b in zip(("xyz_gradient_accum", "denom", "max_radii2D"), got, want):
        a = a.cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: {int((a != b).sum())} elements differ"
    if pattern == "mix" and P >= 63:   # a culled Gaussian with a non-zero gradient row: the row is ignored
        culled = c["radii"] == 0
        assert culled.any() and (np.abs(c["vg"][culled, :2]).max(axis=1) > 0).all()
        assert np.array_equal(got[0].cpu().numpy()[culled], c["acc"][culled])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", PS)
def test_densification_stats_against_the_torch_lines(P, pattern):
    """train.py:134 and gaussian_model.py:693-695 as the reference writes them, on the same device tensors.  The gradient rows of
    culled Gaussians are zero here, as the backward leaves them: the reference's line adds the norm of every row."""
    c = _case(P, 16, pattern)
    radii = _dev(c["radii"])
    vis = radii > 0
    vg = _dev(c["vg"]) * vis.unsqueeze(1)
    got_acc, got_den, got_mx = _run_densification(c, vg=vg)
    acc_t, den_t, mx_t = _dev(c["acc"]), _dev(c["den"]), _dev(c["mx"])
    mx_t[vis] = torch.max(mx_t[vis], radii[vis])
    norm_t = torch.norm(vg[:, :2], dim=-1, keepdim=True)
    acc_t += norm_t
    den_t += vis.unsqueeze(1)
    assert torch.equal(got_den, den_t) and torch.equal(got_mx, mx_t)
    want64 = c["acc"].astype(np.float64) + norm_t.cpu().numpy().astype(np.float64)
    got = got_acc.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want64)
    bar = 2 * _ulp(norm_t.cpu().numpy()) * (norm_t.cpu().numpy() > 0) + 0.5 * _ulp(got)
    print(f"\nmax err / bar {np.max(err / bar):.3f}; differs from torch's float32 sum in {int((got != acc_t.cpu().numpy()).sum())} of {P}")
    assert np.all(err <= bar)


def _check_means(vm, c, M, with_rest=True):
    want = ref.visible_means(c["radii"], c["opacity"], c["rest"] if with_rest else None)
    assert vm.visibility_filter.dtype == torch.bool and vm.n_visible.dtype == torch.int32 and vm.n_visible.dim() == 0
    assert int(vm.n_visible) == want["n"]
    assert np.array_equal(vm.visibility_filter.cpu().numpy(), want["mask"])
    alpha, sh = float(vm.alpha_mean), float(vm.sh_abs_mean) if with_rest else None
    assert vm.alpha_mean.dim() == 0 and vm.alpha_mean.dtype == torch.float32
    if want["n"] == 0:
        assert np.isnan(alpha) and (sh is None or np.isnan(sh))
        return
    e_a = abs(alpha - want["alpha_mean"])
    bar_a = ref.SIGMOID_REL * want["alpha_mean"] + _ulp(want["alpha_mean"])
    print(f"\nalpha_mean err {e_a:.3e} (bar {bar_a:.3e})", end="")
    assert e_a <= bar_a
    if not with_rest:
        return
    if M == 1:
        assert np.isnan(sh)
    else:
        e_s = abs(sh - want["sh_abs_mean"])
        print(f"; sh_abs_mean err {e_s:.3e} (bar {_ulp(want['sh_abs_mean']):.3e})", end="")
        assert e_s <= _ulp(want["sh_abs_mean"])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("P", PS)
def test_visible_means(P, M, pattern):
    c = _case(P, M, pattern)
    radii, opacity, rest = _dev(c["radii"]), _dev(c["opacity"]), _dev(c["rest"])
    vm = ts.visible_means(radii, opacity=opacity, features_rest=rest)
    _check_means(vm, c, M)
    assert vm.sh_abs_mean.requires_grad is False and vm.alpha_mean.requires_grad is False
    again = ts.visible_means(radii, opacity=opacity, features_rest=rest)   # run to run: the same bits
    for a, b in zip(vm, again):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("M", (2, 16))
def test_visible_means_of_an_unaligned_view_and_of_parts(M):
    """features_rest that does not start on a 16-byte boundary takes the 4-byte walk; each mean can be asked for alone."""
    P = 3 * 256 + 5
    c = _case(P, M, "mix")
    big = torch.zeros((P + 1, M - 1, 3), device="cuda")
    big[1:] = _dev(c["rest"])
    rest = big[1:]
    assert rest.is_contiguous() and rest.data_ptr() % 16 != 0
    radii, opacity = _dev(c["radii"]), _dev(c["opacity"])
    _check_means(ts.visible_means(radii, opacity=opacity, features_rest=rest), c, M)
    only_alpha = ts.visible_means(radii, opacity=opacity)
    assert only_alpha.sh_abs_mean is None
    _check_means(only_alpha, c, M, with_rest=False)
    only_sh = ts.visible_means(radii, features_rest=_dev(c["rest"]))
    both = ts.visible_means(radii, opacity=opacity, features_rest=_dev(c["rest"]))
    assert only_sh.alpha_mean is None and torch.equal(_bits(only_sh.sh_abs_mean), _bits(both.sh_abs_mean))
    bare = ts.visible_means(radii)
    assert bare.alpha_mean is None and bare.sh_abs_mean is None and torch.equal(bare.visibility_filter, both.visibility_filter)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", PS)
def test_alpha_regul_backward_through_autograd(P, pattern):
    c = _case(P, 2, pattern)
    lam = 0.37
    opacity = torch.nn.Parameter(_dev(c["opacity"]))
    opacity.grad = _dev(c["grad0"])
    vm = ts.visible_means(_dev(c["radii"]), opacity=opacity, features_rest=_dev(c["rest"]))
    assert vm.alpha_mean.requires_grad and not vm.sh_abs_mean.requires_grad
    (lam * vm.alpha_mean).backward()
    got = opacity.grad.cpu().numpy()
    n = int((c["radii"] > 0).sum())
    culled = c["radii"] <= 0
    assert np.array_equal(got[culled].view(np.uint32), c["grad0"][culled].view(np.uint32))   # n == 0: every row
    if n == 0:
        return
    inc = ref.alpha_regul_increment(c["radii"], c["opacity"], F32(lam), n).reshape(P, 1)
    err = np.abs(got.astype(np.float64) - (c["grad0"].astype(np.float64) + inc))
    bar = ref.ALPHA_TERM_REL * np.abs(inc) + 0.5 * _ulp(got)
    print(f"\nmax err / bar {np.max(err[~culled] / bar[~culled]):.3f}")
    assert np.all(err[~culled] <= bar[~culled])
    assert np.any(got[~culled] != c["grad0"][~culled])   # something was added


def _three_calls(c, M):
    """The three calls through the low-level layer on fresh tensors -> everything they produce."""
    from diff_gaussian_rasterization import _C
    radii, opacity, rest = _dev(c["radii"]), _dev(c["opacity"]), _dev(c["rest"])
    vis, n, alpha, sh = _C.visible_means(radii, opacity, rest)
    grad = _dev(c["grad0"])
    _C.alpha_regul_backward(radii, opacity, torch.full((), 0.37, device="cuda"), n, grad)
    acc, den, mx = _dev(c["acc"]), _dev(c["den"]), _dev(c["mx"])
    _C.densification_stats(_dev(c["vg"]), radii, acc, den, mx)
    return [vis, n, alpha, sh, grad, acc, den, mx]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_both_bindings_give_identical_bits(pattern):
    from diff_gaussian_rasterization import _C
    P, M = 3 * 256 + 5, 16
    c = _case(P, M, pattern)
    outs = {}
    was = _C.binding()
    try:
        for name in ("ctypes", "torch"):
            _C.set_binding(name)
            assert _C.binding() == name
            outs[name] = _three_calls(c, M)
    finally:
        _C.set_binding(was)
    for a, b in zip(outs["ctypes"], outs["torch"]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def test_capture_in_a_graph_and_replay_with_new_contents():
    """The three calls captured once (a single chain: no parallel branches), replayed twice with other input contents; the
    results equal those of direct calls on the same contents."""
    from diff_gaussian_rasterization import _C
    P, M = 257, 16
    cases = [_case(P, M, "mix", salt=s) for s in (0, 1, 2)]
    keys = ("radii", "opacity", "rest", "vg", "grad0", "acc", "den", "mx")
    static = {k: _dev(cases[0][k]) for k in keys}
    upstream = torch.full((), 0.37, device="cuda")

    def calls():
        vis, n, alpha, sh = _C.visible_means(static["radii"], static["opacity"], static["rest"])
        _C.alpha_regul_backward(static["radii"], static["opacity"], upstream, n, static["grad0"])
        _C.densification_stats(static["vg"], static["radii"], static["acc"], static["den"], static["mx"])
        return vis, n, alpha, sh

    side = torch.cuda.Stream()   # warm-up off the default stream, as capture requires
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vis, n, alpha, sh = calls()
    for c in cases[1:]:
        for k in keys:
            static[k].copy_(_dev(c[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = [vis, n, alpha, sh, static["grad0"], static["acc"], static["den"], static["mx"]]
        for name, a, b in zip(("mask", "n", "alpha", "sh", "grad", "acc", "den", "mx"), got, _three_calls(c, M)):
            assert torch.equal(_bits(a), _bits(b)), name


class _Model:
    pass


def test_short_training_loop_against_the_torch_lines():
    """20 iterations on a synthetic scene (P = 3000, 64 x 64, 4 cameras): the existing render and backward, then the new calls,
    compared at every step with the reference's torch lines on cloned accumulators, to the bars of the tests above; the
    rasterizer's own outputs are not touched by the statistics."""
    import diff_gaussian_rasterization as dgr
    W, H, P, lam_alpha = 64, 64, 3000, 0.05
    cams = [ss.make_camera(W, H, 60.0, k) for k in range(4)]
    g = ss.make_gaussians(P, cams[0], seed=5, degree_mode="all3", scale_mu=0.05)
    bg = _dev(np.zeros(3, F32))
    p = {"xyz": _dev(g["means3D"]), "f_dc": _dev(g["sh"][:, :1]), "f_rest": _dev(g["sh"][:, 1:]), "opacity": _dev(g["opacity"]),
         "log_scale": torch.log(_dev(g["scales"])), "rot": _dev(g["rotations"])}
    p = {k: torch.nn.Parameter(v) for k, v in p.items()}
    degrees = _dev(g["degrees"])
    opt = torch.optim.Adam([{"params": [v], "lr": 1e-2} for v in p.values()], eps=1e-15)
    targets = [torch.rand((3, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(k)) for k in range(4)]
    pc, pc_t = _Model(), _Model()
    for m in (pc, pc_t):
        m.xyz_gradient_accum, m.denom, m.max_radii2D = (torch.zeros((P, 1), device="cuda"), torch.zeros((P, 1), device="cuda"),
                                                        torch.zeros(P, device="cuda"))
    seen = 0
    for step in range(20):
        c = cams[step % 4]
        rs = dgr.GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, bg, 1.0, _dev(c.world_view_transform),
                                               _dev(c.full_proj_transform), 3, _dev(c.camera_center), False, False)
        means2D = torch.zeros_like(p["xyz"], requires_grad=True) + 0
        means2D.retain_grad()
        color, radii = dgr.GaussianRasterizer(rs)(
            means3D=p["xyz"], means2D=means2D, shs=torch.cat([p["f_dc"], p["f_rest"]], 1), degrees=degrees, colors_precomp=None,
            opacities=torch.sigmoid(p["opacity"]), scales=torch.exp(p["log_scale"]),
            rotations=torch.nn.functional.normalize(p["rot"]), cov3D_precomp=None, lambda_sh_sparsity=0.0)
        color0, radii0 = color.detach().clone(), radii.clone()
        vm = ts.visible_means(radii, opacity=p["opacity"], features_rest=p["f_rest"])
        opt.zero_grad(set_to_none=True)
        ((color - targets[step % 4]).abs().mean() + lam_alpha * vm.alpha_mean).backward()
        vg0 = means2D.grad.clone()
        ts.add_densification_stats(pc, means2D, radii)
        # the reference's lines
        vis = radii > 0
        alpha_t = torch.sigmoid(p["opacity"].detach().double())[vis].abs().mean()
        sh_t = p["f_rest"].detach().double()[vis].abs().mean()
        old_acc = pc_t.xyz_gradient_accum.clone()
        pc_t.max_radii2D[vis] = torch.max(pc_t.max_radii2D[vis], radii[vis])
        norm_t = torch.norm(means2D.grad[:, :2], dim=-1, keepdim=True)
        pc_t.xyz_gradient_accum += norm_t
        pc_t.denom += vis.unsqueeze(1)
        n = int(vis.sum())
        seen += n
        assert torch.equal(vm.visibility_filter, vis) and int(vm.n_visible) == n and 0 < n < P
        assert abs(float(vm.alpha_mean) - float(alpha_t)) <= ref.SIGMOID_REL * float(alpha_t) + _ulp(float(alpha_t))
        assert abs(float(vm.sh_abs_mean) - float(sh_t)) <= _ulp(float(sh_t))
        assert torch.equal(pc.denom, pc_t.denom) and torch.equal(pc.max_radii2D, pc_t.max_radii2D)
        got = pc.xyz_gradient_accum.cpu().numpy()
        want64 = old_acc.cpu().numpy().astype(np.float64) + norm_t.cpu().numpy().astype(np.float64)
        nt = norm_t.cpu().numpy()
        assert np.all(np.abs(got - want64) <= 2 * _ulp(nt) * (nt > 0) + 0.5 * _ulp(got)), f"step {step}"
        pc_t.xyz_gradient_accum.copy_(pc.xyz_gradient_accum)   # carry the kernel's sum: each step is compared on its own
        # the rasterizer's outputs are as they were
        assert torch.equal(color.detach(), color0) and torch.equal(radii, radii0) and torch.equal(means2D.grad, vg0)
        assert all(torch.isfinite(v.grad).all() for v in p.values())
        opt.step()
    assert seen > 0 and float(pc.xyz_gradient_accum.max()) > 0
