"""The normal-consistency training step in HIP, as r3dgs_normals' docstring writes it --

    out = render(view, pc, pipe, bg, aux=("depth", "alpha"), aux_grad=True, normals=True, features_geom_grad=True)
    L, _ = r3dgs_normals.normal_consistency(out["normal"], out["depth"], rs, alpha=out["alpha"])
    L.backward()

-- against tests/normals_chain_ref.py, the same step as one float64 autograd graph (pinned on the CPU by
tests/test_normals_chain_cpu.py).  One backward() through render(); compared are the loss (1e-5 absolute, the project's value
bar) and the gradients of _xyz, _opacity, _scaling and _rotation (and of F where there is one), each tensor's largest error
against 1e-4 of its largest reference entry, the project's gradient bar.  The only masking is the pixel weight the loss itself
takes on both sides (normals_chain_ref.safe_weight: the oracle's threshold-ambiguous pixels and their eight neighbours, at
most 10 %); no element of any gradient is left out afterwards.  Measured figures: profiles/normals_gpu_tests.txt."""
import types

import numpy as np
import pytest
import torch

from tests import normals_chain_ref as ncr
from tests.test_aux_grad_gpu import Model, forward_args
from tests.test_feature_maps_gpu import PIPE, view_of

pytestmark = pytest.mark.gpu
F32 = np.float32
VALUE_BAR, GRAD_BAR = 1e-5, 1e-4
AUX = ("depth", "alpha")
PARAMS = (("_xyz", "means3D"), ("_opacity", "opacity"), ("_scaling", "scales"), ("_rotation", "rotations"))
_CASES, _GRAPHS = {}, {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Probe(Model):
    """tests/test_aux_grad_gpu.Model whose activated tensors keep their gradients: what render() hands the two geometry
    functions, and where autograd adds their shares."""

    @property
    def get_scaling(self):
        self.scales = torch.exp(self._scaling)
        if self.scales.requires_grad:
            self.scales.retain_grad()
        return self.scales

    @property
    def get_rotation(self):
        self.rotations = torch.nn.functional.normalize(self._rotation)
        if self.rotations.requires_grad:
            self.rotations.retain_grad()
        return self.rotations


def case(name, mip=False):
    """A named scene on the device: the model, the view, the oracle's state over the device's rects (of the anti-aliased
    parameters when `mip`), the pixel weight; the scene's caps and margins are asserted here.  Built once, never modified."""
    if (name, mip) in _CASES:
        return _CASES[(name, mip)]
    import r3dgs_mip
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    sc = ncr.scene(name)
    H, W, P = sc.H, sc.W, sc.P
    pc, view, bg = Probe(sc.g), view_of(sc.cam, H, W), dev(ncr.BG)
    rs = r3dgs_render._settings(view, pc, PIPE, bg, 1.0)
    g_eff, f, ref_mip = sc.g, None, None
    if mip:   # the parameters the rasterizer is handed, from the device's own maps: the decisions are taken over these
        with torch.no_grad():
            f = r3dgs_mip.filter_3d(pc._xyz, r3dgs_mip.pack_cameras([view], "cuda"))
            s_eff, o_eff = r3dgs_mip.filtered_parameters(pc._scaling, pc._opacity, f)
            o_aa = r3dgs_mip.antialias_opacity(pc._xyz, o_eff, s_eff, pc._rotation, None, rs, raw=True)
            g_eff = dict(sc.g, opacity=o_aa.cpu().numpy(), scales=torch.exp(s_eff).cpu().numpy())
        assert (f > 0).all() and not torch.equal(o_aa, pc._opacity)
        ref_mip = dict(filter_3d=f.cpu().numpy(), antialiasing=True)
    fout = _C._forward_common(None, *forward_args(g_eff, sc.cam, H, W), exact=True)

    def rects_of(radii):
        if not _C.tight_rects():
            return None
        rects = _C.export_rects(P, fout[3]).cpu().numpy()
        rects[radii <= 0] = 0
        return rects
    st, amb = ncr.oracle_state(sc, rects_of, opacity=g_eff["opacity"], scales=g_eff["scales"])
    arrays = dict(means3D=sc.g["means3D"], opacity=sc.g["opacity"], scales=pc._scaling.detach().cpu().numpy(),
                  rotations=pc._rotation.detach().cpu().numpy())
    leaves = ncr.as_leaves(arrays)   # the maps' graph without user features: checked here, differentiated by `reference`
    _GRAPHS[(name, mip, False)] = (leaves, ncr.chain_maps(st, leaves, sc.cam, H, W, raw=True, mip=ref_mip))
    flagged, off, weight = ncr.check_scene(sc, st, amb, maps=_GRAPHS[(name, mip, False)][1])
    print(f"normals chain: gpu scene {name}{' + mip' if mip else ''}: flagged {flagged:.4f}, weight 0 on {off:.4f} of the pixels")
    c = types.SimpleNamespace(name=name + (" + mip" if mip else ""), key=(name, mip), sc=sc, H=H, W=W, P=P, pc=pc, view=view, bg=bg, rs=rs,
                              st=st, weight=weight, w=dev(weight), arrays=arrays, f=f, ref_mip=ref_mip)
    _CASES[(name, mip)] = c
    return c


def features_of(c, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (c.P, 2)).astype(F32), (rng.uniform(-1, 1, (2, c.H, c.W)) / (c.H * c.W)).astype(F32)


def step(c, scale_by_alpha=True, F=None, up=None, **replace):
    """The step of the module's docstring, once -> (loss, out); the gradients are left on the model's leaves (and on F)."""
    import r3dgs_normals as rn
    import r3dgs_render
    for t in c.pc.leaves():
        t.grad = None
    kw = dict(aux=AUX, aux_grad=True, normals=True, features_geom_grad=True)
    if F is not None:
        kw["features"] = F
    if c.f is not None:
        kw.update(antialiasing=True, filter_3d=c.f)
    kw.update(replace)
    out = r3dgs_render.render(c.view, c.pc, PIPE, c.bg, **kw)
    L, _ = rn.normal_consistency(out["normal"], out["depth"], c.rs, alpha=out["alpha"], scale_by_alpha=scale_by_alpha, pixel_weight=c.w)
    if F is not None:
        L = L + (out["features"] * up).sum()
    L.backward()
    return L.detach(), out


def reference(c, scale_by_alpha, F=None, up=None):
    """chain_grads(raw=True) of the case.  The maps' graph is built once per (scene, features) and shared by the losses put on
    it (both values of scale_by_alpha); nothing in it is modified."""
    key = c.key + (F is not None,)
    if key not in _GRAPHS:
        leaves = ncr.as_leaves(dict(c.arrays, features=F))
        _GRAPHS[key] = (leaves, ncr.chain_maps(c.st, leaves, c.sc.cam, c.H, c.W, raw=True, features=leaves.get("features"), mip=c.ref_mip))
    leaves, maps = _GRAPHS[key]
    return ncr.grads_of(ncr.loss_of_maps(maps, c.sc.cam, scale_by_alpha=scale_by_alpha, pixel_weight=c.weight, feature_upstream=up), leaves)


def hold(what, loss, got, want):
    """Every figure is printed before anything is asserted."""
    lines, failures = [], []
    err = abs(float(loss) - want["loss"])
    lines.append(f"normals chain: gpu, {what}: loss {float(loss):.6f} (ref {want['loss']:.6f}), error {err:.2e} (bar {VALUE_BAR})")
    if not err <= VALUE_BAR:
        failures.append(lines[-1])
    for name, g in got.items():
        assert g is not None, f"{what}: {name} received no gradient"
        a, b = g.detach().cpu().numpy().astype(np.float64), want[name]
        top, e = np.abs(b).max(), np.abs(a - b.reshape(a.shape)).max()
        lines.append(f"normals chain: gpu, {what}: d_{name} {e / top:.2e} of max|ref| {top:.3e} (bar {GRAD_BAR})")
        if not (top > 0 and e <= GRAD_BAR * top):
            failures.append(lines[-1])
    print("\n".join(lines))
    assert not failures, "\n".join(failures)


def model_grads(c):
    return {ref_name: getattr(c.pc, attr).grad for attr, ref_name in PARAMS}


@pytest.mark.parametrize("name,scale_by_alpha", [("landscape", True), ("landscape", False), ("portrait", True)])
def test_the_step_against_the_float64_chain(name, scale_by_alpha):
    c = case(name)
    L, _ = step(c, scale_by_alpha)
    hold(f"{c.name} scale_by_alpha={scale_by_alpha}", L, model_grads(c), reference(c, scale_by_alpha))


def test_the_step_with_user_features_in_front_of_the_normals():
    """features=F (C = 2) rides the same launch in front of the three normal channels, with a loss term of its own: the channel
    offsets of the upstream gradient and of dL/dF."""
    c = case("landscape")
    F0, up = features_of(c)
    F = dev(F0).requires_grad_(True)
    L, out = step(c, True, F, dev(up))
    assert out["features"].shape == (2, c.H, c.W) and out["normal"].shape == (3, c.H, c.W)
    hold(f"{c.name} with features C=2", L, dict(model_grads(c), features=F.grad), reference(c, True, F0, up))


def test_the_step_behind_both_mip_filters():
    """antialiasing=True, filter_3d=f over the one camera: both maps in front of the whole step.  The state, the margins and
    the pixel weight are those of the anti-aliased parameters; the reference takes the normals from the unfiltered scales."""
    c = case("landscape", mip=True)
    L, _ = step(c, True)
    hold(c.name, L, model_grads(c), reference(c, True))


def _ulp(x):
    return np.spacing(np.abs(x).astype(F32)).astype(np.float64)


def test_the_routes_add_up_bit_for_bit():
    """The gradient of the step with every keyword on against three backward runs that leave one route open each:
        A  features_geom_grad=False, aux_grad=False            the normals' own backward: the rotation alone
        B  features_geom_grad only, the normals detached       the blend weights of the three channels
        C  aux_grad only, the normal map detached              depth and alpha
    render() hands B's and C's functions the SAME tensors: _xyz and _opacity themselves, exp(_scaling) and
    normalize(_rotation) built once.  So autograd adds B's and C's shares there -- two addends, any order gives the same bits --
    sends the sums through exp / normalize once, and adds A's share at the rotation leaf (two addends again).  Rebuilt in that
    order from the three runs, every tensor equals the full step with torch.equal.
    The plain sum of the three runs' LEAF gradients has another order for _scaling and _rotation (the activation's backward
    is applied to each share, then added): it is compared within 4 ulp of the largest addend, where for the rotation the
    shares at normalize()'s output, divided by |q|, count as addends too -- the projection g - u (u . g) rounds at the size of
    g, not of what is left of it."""
    import r3dgs_normals as rn
    import r3dgs_render
    c = case("landscape")
    pc = c.pc
    zero = torch.zeros_like

    def run(loss_of, **kw):
        for t in pc.leaves():
            t.grad = None
        pc.scales = pc.rotations = None
        out = r3dgs_render.render(c.view, pc, PIPE, c.bg, aux=AUX, **kw)
        L = loss_of(out)
        L.backward()
        leaf = {a: (zero(getattr(pc, a)) if getattr(pc, a).grad is None else getattr(pc, a).grad.clone()) for a, _ in PARAMS}
        act = {k: (None if t is None or t.grad is None else t.grad.clone()) for k, t in (("scales", pc.scales), ("rotations", pc.rotations))}
        return L.detach(), leaf, act

    def loss(N, d, a):
        return rn.normal_consistency(N, d, c.rs, alpha=a, pixel_weight=c.w)[0]
    L, full, _ = run(lambda o: loss(o["normal"], o["depth"], o["alpha"]), aux_grad=True, normals=True, features_geom_grad=True)
    LA, A, _ = run(lambda o: loss(o["normal"], o["depth"], o["alpha"]), normals=True)
    with torch.no_grad():
        n = rn.gaussian_normals(pc._xyz, pc._scaling, pc._rotation, c.rs, raw=True)
    LB, B, Bact = run(lambda o: loss(o["features"], o["depth"], o["alpha"]), features=n, features_geom_grad=True)
    LC, C, Cact = run(lambda o: loss(o["normal"].detach(), o["depth"], o["alpha"]), aux_grad=True, normals=True)
    assert torch.equal(L, LA) and torch.equal(L, LB) and torch.equal(L, LC), "the four runs see different maps"
    for a in ("_xyz", "_opacity", "_scaling"):
        assert not A[a].any(), f"run A reached {a}"
    for runs, name in ((B, "B"), (C, "C")):
        for a, _ in PARAMS:
            assert runs[a].any(), f"run {name} left {a} without a gradient"
    assert A["_rotation"].any()
    for a in ("_xyz", "_opacity"):
        assert torch.equal(full[a], B[a] + C[a]), f"{a}: the full step is not B + C"
    ls, q = pc._scaling.detach().clone().requires_grad_(True), pc._rotation.detach().clone().requires_grad_(True)
    d_ls, = torch.autograd.grad(torch.exp(ls), ls, Bact["scales"] + Cact["scales"])
    d_q, = torch.autograd.grad(torch.nn.functional.normalize(q), q, Bact["rotations"] + Cact["rotations"])
    assert torch.equal(full["_scaling"], d_ls), "_scaling: not exp's backward of B's + C's share"
    assert torch.equal(full["_rotation"], A["_rotation"] + d_q), "_rotation: not A + normalize's backward of B's + C's share"
    norm = pc._rotation.detach().norm(dim=1, keepdim=True)
    extra = {"_scaling": [], "_rotation": [Bact["rotations"] / norm, Cact["rotations"] / norm]}
    for a, shares in ((("_scaling"), (B, C)), ("_rotation", (A, B, C))):
        plain = sum(s[a] for s in shares)
        addends = [s[a].abs().amax(1, keepdim=True) for s in shares] + [t.abs().amax(1, keepdim=True) for t in extra[a]]
        largest = torch.stack(addends).amax(0).cpu().numpy()
        diff = (full[a].double() - plain.double()).abs().cpu().numpy()
        worst = float((diff / _ulp(largest)).max())
        print(f"normals chain: gpu, routes: {a}: full step against the plain sum of the leaf gradients: {worst:.2f} ulp of the largest addend (bar 4)")
        assert worst <= 4.0, (a, worst)


def test_the_step_twice_gives_the_same_bits():
    c = case("landscape")
    F0, up = features_of(c)
    runs = []
    for _ in range(2):
        F = dev(F0).requires_grad_(True)
        L, out = step(c, True, F, dev(up))
        runs.append([L, out["normal"].detach(), out["depth"].detach(), out["alpha"].detach(), F.grad.clone()] +
                    [getattr(c.pc, a).grad.clone() for a, _ in PARAMS])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs of the step, different bits"


@pytest.mark.parametrize("mip", [False, True])
def test_a_colour_backward_after_the_step_is_the_one_before_it(mip):
    """The step replays the forward's state twice (feature launch, aux launch) and walks it backwards twice: the blobs are only
    read, so the colour backward of a later render is bit for bit the one of an earlier render."""
    import r3dgs_render
    c = case("landscape", mip=mip)
    wimg = dev(np.linspace(0.5, 1.5, 3 * c.H * c.W, dtype=F32).reshape(3, c.H, c.W))
    extra = dict(antialiasing=True, filter_3d=c.f) if mip else {}

    def colour():
        for t in c.pc.leaves():
            t.grad = None
        out = r3dgs_render.render(c.view, c.pc, PIPE, c.bg, **extra)
        (out["render"] * wimg).sum().backward()
        return [out["render"].detach()] + [t.grad.clone() for t in c.pc.leaves()] + [out["viewspace_points"].grad.clone()]
    before = colour()
    step(c, True)
    for a, b in zip(before, colour()):
        assert torch.equal(a, b), "the step changed a later colour backward"
