"""GPU tests (-m gpu) of the depth-distortion map and the gradients through it (include/r3dgs_distortion.h,
csrc/distortion.hip) against the float64 reference tests/distortion_ref.py over the oracle re-binned into the HIP rects.

Bars: value |got - ref| <= 1e-5 * max(1, max |ref map|) off the flagged pixels; gradients max |got - ref| <= 1e-4 * max |ref|
per tensor.  Flagged = the oracle's threshold-ambiguous pixels, at most 0.1 %; they carry a zero upstream gradient on both
sides.  The measured worst values are printed (profiles/distortion_gpu_tests.txt keeps a copy)."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aux_ref as ar
from tests import distortion_ref as dr

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
BG = np.array([0.1, 0.3, 0.2], np.float32)
REL = 1e-4
VAL = 1e-5
FLAG_MAX_FRACTION = 1e-3
NAMES = ("means2D", "means3D", "opacity", "scales", "rotations")
LIN = (0.0, 0.0)
NF = (0.2, 50.0)


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


def dev(a):
    return EMPTY if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def forward_args(g, cam, H, W, scales=None, rotations=None):
    return (dev(BG), dev(g["means3D"]), EMPTY, dev(g["opacity"]), dev(g["scales"]) if scales is None else scales,
            dev(g["rotations"]) if rotations is None else rotations, 1.0, EMPTY, dev(cam.world_view_transform),
            dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, H, W, dev(g["sh"]), dev(g["degrees"]), dev(cam.camera_center),
            False, False)


def fwd(C_, P, H, W, fout, mapping=LIN, moments=True):
    R, _, _, geom, binning, img = fout
    return C_.distortion_map(P, R, H, W, geom, binning, img, *mapping, want_moments=moments)


def bwd(C_, g, cam, H, W, fout, up, moments, mapping=LIN, want=None, cov=None):
    R, _, radii, geom, binning, img = fout
    return C_.distortion_map_backward(len(g["means3D"]), R, H, W, geom, binning, img, dev(cam.world_view_transform),
                                      dev(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, dev(g["means3D"]),
                                      EMPTY if cov is not None else dev(g["scales"]), 1.0,
                                      EMPTY if cov is not None else dev(g["rotations"]), EMPTY if cov is None else dev(cov), radii,
                                      None if up is None else dev(up), moments, *mapping, **({} if want is None else {"want": want}))


def upstream(H, W, seed, ok=None):
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, H * W).astype(np.float32)
    return g if ok is None else g * ok.reshape(-1)


def held(got, ref, what, names=NAMES):
    for k in names:
        a, b = got[k].cpu().numpy().astype(np.float64), np.asarray(ref[k], np.float64)
        if k == "means2D":
            assert not a[:, 2].any()
            a = a[:, :2]
        scale = np.abs(b).max()
        err = np.abs(a - b.reshape(a.shape)).max()
        print(f"[distortion grad {what}] {k}: max err {err:.3e}, bar {REL * scale:.3e} (max |ref| {scale:.3e})")
        assert scale > 0 and err <= REL * scale, (what, k, err, scale)


class Case:
    """A scene, its exact-size forward on the device, the oracle's state over the device's rects and the unflagged pixels."""

    def __init__(self, C_, cam, g, H, W):
        self.cam, self.g, self.H, self.W, self.P = cam, g, H, W, len(g["means3D"])
        self.fout = C_._forward_common(None, *forward_args(g, cam, H, W), exact=True)
        ref = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                          cam.full_proj_transform, cam.tanfovx, cam.tanfovy, H, W, g["sh"], g["degrees"], cam.camera_center,
                          want_ambig=True)
        if C_.tight_rects():
            rects = C_.export_rects(self.P, self.fout[3]).cpu().numpy()
            rects[ref["radii"] <= 0] = 0
            ref = orc.with_rects(ref, rects, want_ambig=True)
        self.st = ref["state"]
        amb = ref["ambig"].reshape(-1) != 0
        assert amb.mean() <= FLAG_MAX_FRACTION
        self.okb = ~amb
        self.ok = self.okb.astype(np.float32)
        self._refs = {}

    def ref(self, up, mapping, seed):
        key = (mapping, seed)
        if key not in self._refs:   # computed once, shared, never modified
            g, cam = self.g, self.cam
            self._refs[key] = dr.reference_grads(self.st, g["means3D"], g["opacity"], g["scales"], g["rotations"],
                                                 cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy, up,
                                                 *mapping)
        return self._refs[key]

    def check(self, C_, what, mapping=LIN, seed=31):
        """The map and every gradient against the reference."""
        up = upstream(self.H, self.W, seed, self.ok)
        ref = self.ref(up, mapping, seed)
        dist, mom = fwd(C_, self.P, self.H, self.W, self.fout, mapping)
        assert dist.shape == (1, self.H, self.W) and mom.shape == (2, self.H, self.W) and dist.dtype == torch.float32
        want = ref["map"]
        bar = VAL * max(1.0, np.abs(want).max())
        err = np.abs(dist.reshape(-1).cpu().numpy().astype(np.float64) - want)[self.okb].max()
        print(f"[distortion {what} {mapping}] value error {err:.3e}, bar {bar:.3e} (max |ref| {np.abs(want).max():.3e})")
        assert np.abs(want).max() > 0 and err <= bar, (what, err, bar)
        empty = (np.asarray(self.st["n_contrib"]).reshape(-1) == 0) & self.okb
        assert not dist.reshape(-1).cpu().numpy()[empty].any()
        held(bwd(C_, self.g, self.cam, self.H, self.W, self.fout, up, mom, mapping), ref, f"{what} {mapping}")
        return dist, mom


@pytest.fixture(scope="module")
def scene_a(C_):
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    return Case(C_, cam, g, kw["H"], kw["W"])


@pytest.mark.parametrize("mapping", [LIN, NF])
def test_scene_a_against_the_reference(C_, scene_a, mapping):
    """Scene A (P = 2000, 100x70), both mappings, both settings of set_f64_chain."""
    was = C_.set_f64_chain(True)
    try:
        for f64 in (True, False):
            C_.set_f64_chain(f64)
            scene_a.check(C_, f"scene A f64_chain={f64}", mapping)
    finally:
        C_.set_f64_chain(was)


@pytest.mark.parametrize("name", ["17x17", "portrait", "stacked512", "stacked203", "FAR"])
def test_edge_scenes_against_the_reference(C_, name):
    """17x17 (one pixel past a tile), portrait with fx != fy, lists longer than one 64-entry chunk (P = 512: three chunks; P = 203:
    a partial last chunk), and FAR: depths in 100 .. 104 under a narrow field of view, which raw fp32 moments cannot pass."""
    cam, g, H, W, _ = next(s[1:] for s in dr.gpu_scenes() if s[0] == name)
    c = Case(C_, cam, g, H, W)
    if name.startswith("stacked") or name == "FAR":
        ex = C_.export_binning(c.P, c.fout[0], H, W, c.fout[3], c.fout[4], c.fout[5])
        deepest = int(ex["n_contrib"].max())
        print(f"[distortion {name}] deepest contributor {deepest}")
        assert deepest > (128 if name == "stacked512" else 64)
    if name == "FAR":
        z = c.st["depths"][c.st["radii"] > 0]
        assert z.min() > 99.5 and z.max() < 104.5
    c.check(C_, name)


def test_small_models_on_a_17x19_image(C_):
    """P = 65 (one Gaussian past a wave) on 17x19, partial tiles on both axes: map and gradients against the reference, both
    mappings.  P = 1: a single Gaussian has no pair j < k, so the map is zero (held to the value bar, which is absolute there) and
    so is every gradient in exact arithmetic.  The kernels work on depths shifted by a per-pixel reference (distortion_math.h
    mapped_depth_shifted) and form the gradient from the residues A m - S1 and (A m - 2 S1) m + S2; whether those vanish bit for
    bit is the kernel's business, so the gradients are printed and held to be finite, of P rows and the same bits in two runs."""
    kw = ar.SMALL["P65_17x19"]
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    c.check(C_, "P65 17x19", LIN)
    c.check(C_, "P65 17x19", NF)
    kw = ar.SMALL["P1_17x19"]
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    assert int(np.asarray(c.st["n_contrib"]).max()) == 1, "the one Gaussian must be blended"
    for mapping in (LIN, NF):
        dist, mom = fwd(C_, 1, c.H, c.W, c.fout, mapping)
        err = float(dist.abs().reshape(-1)[torch.from_numpy(c.okb).cuda()].max())
        print(f"[distortion P1 17x19 {mapping}] max |map| {err:.3e} (bar {VAL:.1e}), max |moments| {float(mom.abs().max()):.3e}")
        assert err <= VAL and mom.shape == (2, c.H, c.W)
        up = upstream(c.H, c.W, 33, c.ok)
        a, b = (bwd(C_, g, cam, c.H, c.W, c.fout, up, mom, mapping, want=C_.AUX_GRADS) for _ in range(2))
        for k in C_.AUX_GRADS:
            print(f"[distortion P1 17x19 {mapping}] {k}: max |gradient| {float(a[k].abs().max()):.3e} (exact arithmetic: 0)")
            assert a[k].shape[0] == 1 and bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k


def test_precomputed_covariance(C_):
    kw = ar.SCENE_17
    cam, g, _ = ar.make_scene(kw)
    c = Case(C_, cam, g, kw["H"], kw["W"])
    q, S = g["rotations"].astype(np.float64), g["scales"].astype(np.float64)
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = Rm * S[:, None, :]
    Sig = L @ L.transpose(0, 2, 1)
    cov = np.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1).astype(np.float32)
    args = list(forward_args(g, cam, c.H, c.W))
    args[4], args[5], args[7] = EMPTY, EMPTY, dev(cov)
    fout = C_._forward_common(None, *args, exact=True)
    assert torch.equal(fout[2] > 0, c.fout[2] > 0), "the two forwards must see the same splats"
    up = upstream(c.H, c.W, 32, c.ok)
    _, mom = fwd(C_, c.P, c.H, c.W, fout)
    got = bwd(C_, g, cam, c.H, c.W, fout, up, mom, want=C_.AUX_GRADS, cov=cov)
    ref = dr.reference_grads(c.st, g["means3D"], g["opacity"], None, None, cam.world_view_transform, cam.full_proj_transform,
                             cam.tanfovx, cam.tanfovy, up, cov3D_precomp=cov)
    assert not got["scales"].any() and not got["rotations"].any()
    held(got, ref, "cov3D_precomp", ("means2D", "means3D", "opacity", "cov3D"))


def test_every_forward_path_leaves_the_same_map(C_, golden_dir):
    """Exact, reserved (twice: the second is the replayed one), lean blob, raw parameters; ragged inference against quantised."""
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    P, H, W = kw["P"], kw["H"], kw["W"]
    scaling, rotation = dev(np.log(g["scales"]).astype(np.float32)), dev(g["rotations"])
    scales, rotations = C_.activate_params(scaling, rotation)
    args = forward_args(g, cam, H, W, scales, rotations)
    exact = C_._forward_common(None, *args, exact=True)
    want = fwd(C_, P, H, W, exact, NF)
    assert float(want[0].max()) > 0

    def same(fout, what):
        got = fwd(C_, P, H, W, fout, NF)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    reserve = int(exact[0].pairs * 1.25) + 4096
    for _ in range(2):
        reserved = C_._forward_common(None, *args, exact=False, _reserve=reserve)
        assert reserved[0].ticket > 0, "the reserved path was not taken"
        same(reserved, "reserved")
    C_.hint_next_forward(False)
    lean = C_._forward_common(None, *args, exact=True)
    C_.hint_next_forward(True)
    full = C_._forward_common(None, *args, exact=True)
    assert lean[3].numel() < full[3].numel(), "the hint did not select the lean blob"
    same(lean, "lean")
    same(full, "full")
    sh = dev(g["sh"])
    params = C_.rasterize_gaussian_params(args[0], args[1], sh[:, :1].contiguous(), sh[:, 1:].contiguous(), args[15], args[3],
                                          scaling, rotation, 1.0, args[8], args[9], cam.tanfovx, cam.tanfovy, H, W, args[16],
                                          False, False, exact=True)
    same(params, "raw parameters")
    from r3dgs_quantised import QuantisedModel
    from tests import test_quantised_gpu as tq
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    c = tq.camera("131x77", T=(0.1, -0.05, 4.0))
    ragged = fwd(C_, qm.P, c.H, c.W, tq.ragged_forward(C_, qm, tq.ragged_inputs(C_, qm), c))
    quant = fwd(C_, qm.P, c.H, c.W, tq.quantised_forward(C_, qm, c))
    assert float(ragged[0].max()) > 0
    assert torch.equal(ragged[0], quant[0]) and torch.equal(ragged[1], quant[1])


def test_empty_model_all_culled_and_bad_mapping(C_):
    H, W = 40, 56
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=64, W=W, H=H))
    empty = {k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()}
    fout = C_._forward_common(None, *forward_args(empty, cam, H, W), exact=True)
    dist, mom = fwd(C_, 0, H, W, fout)
    assert dist.shape == (1, H, W) and dist.is_cuda and not dist.any() and not mom.any()
    got = bwd(C_, empty, cam, H, W, fout, upstream(H, W, 33), mom)
    assert all(t.shape[0] == 0 for t in got.values())
    behind = dict(g)
    behind["means3D"] = g["means3D"].copy()
    behind["means3D"][:, 2] = -np.abs(g["means3D"][:, 2]) - 1.0
    fout = C_._forward_common(None, *forward_args(behind, cam, H, W), exact=True)
    assert int(fout[0]) == 0 and not fout[2].any()
    dist, mom = fwd(C_, 64, H, W, fout)
    assert not dist.any() and not mom.any()
    for k, t in bwd(C_, behind, cam, H, W, fout, upstream(H, W, 33), mom).items():
        assert t.shape[0] == 64 and not t.any(), k
    for bad in ((1.0, 0.5), (0.0, 5.0), (-1.0, 2.0), (2.0, 2.0)):
        with pytest.raises(ValueError):
            C_.distortion_map(64, fout[0], H, W, fout[3], fout[4], fout[5], *bad)
    # straight at the C ABI: a negative status and a message
    import ctypes
    out = torch.zeros(H * W, device="cuda")
    rc = C_._lib.r3dgs_distortion_map(64, 0, W, H, None, None, None, 1.0, 0.5, out.data_ptr(), None,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc < 0 and b"near" in C_._lib.r3dgs_last_error()


def test_overflowed_reservation_gives_zero_gradients(C_, scene_a):
    """A forward whose reservation is too small drops the farthest pairs: a Gaussian that lost pairs gets zero gradients."""
    c = scene_a
    args = forward_args(c.g, c.cam, c.H, c.W)
    need = int(c.fout[0].pairs)
    reserve = need // 2
    C_.hint_next_forward(True)
    fout = C_._forward_common(None, *args, exact=False, _reserve=reserve, _strict_override=False)
    assert fout[0].truncated, "the reservation did not overflow"
    dist, mom = fwd(C_, c.P, c.H, c.W, fout)
    got = bwd(C_, c.g, c.cam, c.H, c.W, fout, upstream(c.H, c.W, 34), mom)
    ex = C_.export_binning(c.P, fout[0], c.H, c.W, fout[3], fout[4], fout[5])
    kept = torch.bincount(ex["point_list"][:fout[0].capacity].long().clamp(max=c.P), minlength=c.P + 1)[:c.P]
    wanted = torch.bincount(C_.export_binning(c.P, c.fout[0], c.H, c.W, c.fout[3], c.fout[4], c.fout[5])["point_list"].long(),
                            minlength=c.P)[:c.P]
    lost = (kept < wanted) & (c.fout[2] > 0)
    assert lost.any() and (~lost & (wanted > 0)).any()
    for k, t in got.items():
        assert not t[lost].any(), k
    assert got["means3D"][~lost].abs().max() > 0


def test_each_output_alone_no_upstream_determinism_and_untouched_state(C_, scene_a):
    """want= one at a time equals the full call; a NULL upstream gives zeros; two runs are bit-identical; the three blobs are
    byte-identical after both calls and the colour backward afterwards is the one without them."""
    import synth_scene as ss
    c = scene_a
    g, cam, H, W = c.g, c.cam, c.H, c.W
    args = forward_args(g, cam, H, W)
    (bg, m3, colors, op, sc, rot, mod, cov, vm, pm, tx, ty, _, _, sh, deg, campos, _, _) = args
    dl = dev(ss.upstream_grad(W, H, seed=3) * (W * H))
    up = upstream(H, W, 35)

    def run(with_dist):
        C_.hint_next_forward(True)
        fout = C_._forward_common(None, *args, exact=True)
        R, _, radii, geom, binning, img = fout
        if with_dist:
            before = [t.clone() for t in (geom, binning, img)]
            dist, mom = fwd(C_, c.P, H, W, fout, NF)
            again = fwd(C_, c.P, H, W, fout, NF)
            assert torch.equal(dist, again[0]) and torch.equal(mom, again[1])
            assert torch.equal(fwd(C_, c.P, H, W, fout, NF, moments=False), dist)
            full = bwd(C_, g, cam, H, W, fout, up, mom, NF, want=C_.AUX_GRADS)
            assert float(full["cov3D"].abs().max()) > 0
            for k, t in bwd(C_, g, cam, H, W, fout, up, mom, NF, want=C_.AUX_GRADS).items():
                assert torch.equal(t, full[k]), k
            for k in C_.AUX_GRADS:
                one = bwd(C_, g, cam, H, W, fout, up, mom, NF, want=(k,))
                assert set(one) == {k} and torch.equal(one[k], full[k]), k
            assert bwd(C_, g, cam, H, W, fout, up, mom, NF, want=()) == {}   # no output asked for: nothing comes back
            none = bwd(C_, g, cam, H, W, fout, None, mom, NF)
            assert all(not t.any() for t in none.values())
            for a, b in zip(before, (geom, binning, img)):
                assert torch.equal(a, b), "a state blob was written"
        return C_.rasterize_gaussians_backward(bg, m3, radii, colors, sc, rot, mod, cov, vm, pm, tx, ty, dl, sh, deg, campos, geom,
                                               R, binning, img, 0.0, False)
    plain, after = run(False), run(True)
    for k, (a, b) in enumerate(zip(plain, after)):
        assert torch.equal(a, b), k


def test_captured_forward_and_backward_follow_the_upstream_buffer(C_, scene_a):
    c = scene_a
    first, second = upstream(c.H, c.W, 36), upstream(c.H, c.W, 37)
    R, _, radii, geom, binning, img = c.fout
    fixed = dev(first)
    model = [dev(c.g[k]) for k in ("means3D", "scales", "rotations")]
    vm, pm = dev(c.cam.world_view_transform), dev(c.cam.full_proj_transform)

    def go():
        dist, mom = C_.distortion_map(c.P, R, c.H, c.W, geom, binning, img, *NF, want_moments=True)
        return dist, C_.distortion_map_backward(c.P, R, c.H, c.W, geom, binning, img, vm, pm, c.cam.tanfovx, c.cam.tanfovy, model[0],
                                                model[1], 1.0, model[2], EMPTY, radii, fixed, mom, *NF)
    want_dist, want_first = go()   # warm-up outside the capture (the workspace size is asked here)
    want_first = {k: v.clone() for k, v in want_first.items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_dist, static = go()
    for up in (second, first):
        fixed.copy_(dev(up))
        graph.replay()
        torch.cuda.synchronize()
        _, mom = fwd(C_, c.P, c.H, c.W, c.fout, NF)
        direct = bwd(C_, c.g, c.cam, c.H, c.W, c.fout, up, mom, NF)
        assert torch.equal(static_dist, want_dist)
        for k in direct:
            assert torch.equal(static[k], direct[k]), k
    for k in want_first:
        assert torch.equal(static[k], want_first[k]), k
    _, mom = fwd(C_, c.P, c.H, c.W, c.fout, NF)
    assert not torch.equal(bwd(C_, c.g, c.cam, c.H, c.W, c.fout, second, mom, NF)["means3D"], want_first["means3D"])


class Model:
    """The reference's GaussianModel, as far as render() looks at it."""

    def __init__(self, g):
        sh = dev(g["sh"])
        self._xyz = dev(g["means3D"]).requires_grad_(True)
        self._features_dc = sh[:, :1].contiguous().requires_grad_(True)
        self._features_rest = sh[:, 1:].contiguous().requires_grad_(True)
        self._opacity = dev(g["opacity"]).requires_grad_(True)
        self._scaling = dev(np.log(g["scales"]).astype(np.float32)).requires_grad_(True)
        self._rotation = dev(g["rotations"] * 1.3).requires_grad_(True)
        self._degrees, self.active_sh_degree, self.max_sh_degree = dev(g["degrees"]), 3, 3
        self.act_grads = {}

    get_xyz = property(lambda self: self._xyz)

    def _activated(self, name, t):   # the gradient autograd hands the activated tensor (summed over its users) is kept
        if t.requires_grad:
            t.register_hook(lambda grad: self.act_grads.__setitem__(name, grad.clone()))
        return t

    get_scaling = property(lambda self: self._activated("scales", torch.exp(self._scaling)))
    get_rotation = property(lambda self: self._activated("rotations", torch.nn.functional.normalize(self._rotation)))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))

    def leaves(self):
        return (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation)


def grads_close(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        assert err <= REL * max(scale, 1e-30), (what, k, err, scale)


def scene_view(cam, H, W):
    return NS(image_height=H, image_width=W, FoVx=cam.FoVx, FoVy=cam.FoVy, world_view_transform=dev(cam.world_view_transform),
              full_proj_transform=dev(cam.full_proj_transform), camera_center=dev(cam.camera_center))


PIPE = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


@pytest.mark.parametrize("route", ["fused", "python_sh"])
def test_through_render(C_, route, monkeypatch):
    import r3dgs_render
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    H, W = kw["H"], kw["W"]
    pc, view, bg = Model(g), scene_view(cam, H, W), dev(BG)

    def options():
        if route == "python_sh":
            return dict(override_color=torch.sigmoid(pc._features_dc[:, 0, :]))
        return dict(variable_sh_bands=False)
    assert r3dgs_render.fused_path_applies(pc, PIPE, options().get("override_color")) == (route == "fused")

    def backward_of(loss_of, **kw_):
        for t in pc.leaves():
            t.grad = None
        pc.act_grads = {}
        out = r3dgs_render.render(view, pc, PIPE, bg, **kw_, **options())
        loss_of(out).backward()
        vs = out["viewspace_points"].grad
        out["act_grads"] = dict(pc.act_grads)
        return [torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in pc.leaves()] + [vs.clone()], out

    # the keyword absent: nothing new is launched, the same dictionary
    with monkeypatch.context() as m:
        m.setattr(C_, "distortion_map", None)
        plain = r3dgs_render.render(view, pc, PIPE, bg, **options())
    assert "distortion" not in plain
    wimg = dev(np.linspace(0.5, 1.5, 3 * H * W, dtype=np.float32).reshape(3, H, W))
    wd = dev(np.linspace(0.2, 1.0, H * W, dtype=np.float32).reshape(1, H, W))
    only_render, out_r = backward_of(lambda o: (o["render"] * wimg).sum(), distortion=NF)
    assert out_r["distortion"].requires_grad and out_r["distortion"].shape == (1, H, W)
    assert torch.equal(out_r["render"], plain["render"])
    only_dist, out = backward_of(lambda o: (o["distortion"] * wd).sum(), distortion=NF)
    assert float(only_dist[0].abs().max()) > 0 and float(only_dist[4].abs().max()) > 0 and float(only_dist[-1].abs().max()) > 0
    # image + distortion in one step: the two routes' separate gradients added in autograd's order, bit for bit
    both, _ = backward_of(lambda o: (o["render"] * wimg).sum() + (o["distortion"] * wd).sum(), distortion=NF)
    expect = [a + b for a, b in zip(only_render, only_dist)]
    if route == "python_sh":   # one exp / normalize node feeds both: autograd adds the two gradients in front of it, then chains
        gs = out_r["act_grads"]["scales"] + out["act_grads"]["scales"]
        gr = out_r["act_grads"]["rotations"] + out["act_grads"]["rotations"]
        leaf_s, leaf_r = pc._scaling.detach().clone().requires_grad_(True), pc._rotation.detach().clone().requires_grad_(True)
        expect[4], = torch.autograd.grad(torch.exp(leaf_s), leaf_s, gs)
        expect[5], = torch.autograd.grad(torch.nn.functional.normalize(leaf_r), leaf_r, gr)
    for k, (x, y) in enumerate(zip(both, expect)):
        assert torch.equal(x, y), (route, k)
    # the VALUES: the library call over a forward of the same model, torch's chain rule through exp / normalize by hand
    with torch.no_grad():
        scales, rotations = torch.exp(pc._scaling), torch.nn.functional.normalize(pc._rotation)
        fout = C_.rasterize_gaussian_params(bg, pc._xyz, pc._features_dc, pc._features_rest, pc._degrees, pc._opacity, pc._scaling,
                                            pc._rotation, 1.0, view.world_view_transform, view.full_proj_transform, cam.tanfovx,
                                            cam.tanfovy, H, W, view.camera_center, False, False, exact=True)
        dist, mom = C_.distortion_map(kw["P"], fout[0], H, W, fout[3], fout[4], fout[5], *NF, want_moments=True)
        d = C_.distortion_map_backward(kw["P"], fout[0], H, W, fout[3], fout[4], fout[5], view.world_view_transform,
                                       view.full_proj_transform, cam.tanfovx, cam.tanfovy, pc._xyz, scales, 1.0, rotations, EMPTY,
                                       fout[2], wd, mom, *NF)
    route_dist = out["distortion"].detach()

    def same_as_direct(a, b):   # the raw-parameter forward is the fused route's own; the other route activates in torch (an
        if route == "fused":    # ulp of exp away), so its map is held to the direct one by the value bar instead
            return torch.equal(a, b)
        return float((a - b).abs().max()) <= VAL * max(1.0, float(b.abs().max()))
    assert same_as_direct(route_dist, dist)
    leaf = pc._rotation.detach().clone().requires_grad_(True)
    drot, = torch.autograd.grad(torch.nn.functional.normalize(leaf), leaf, d["rotations"])
    zero = torch.zeros_like
    want = [d["means3D"], zero(pc._features_dc), zero(pc._features_rest), d["opacity"], d["scales"] * scales, drot, d["means2D"]]
    grads_close(only_dist, want, route + ", values")
    # True is the linear mapping; no_grad gives the detached map; it composes with aux / aux_grad / normals
    with torch.no_grad():
        lin = r3dgs_render.render(view, pc, PIPE, bg, distortion=True, **options())["distortion"]
        assert not lin.requires_grad
        assert same_as_direct(lin, C_.distortion_map(kw["P"], fout[0], H, W, fout[3], fout[4], fout[5]))
        assert torch.equal(r3dgs_render.render(view, pc, PIPE, bg, distortion=NF, **options())["distortion"], route_dist)
    mixed = r3dgs_render.render(view, pc, PIPE, bg, distortion=NF, aux=("depth", "alpha"), aux_grad=True, normals=True, **options())
    assert torch.equal(mixed["distortion"], route_dist) and mixed["distortion"].requires_grad and mixed["depth"].requires_grad
    assert mixed["normal"].shape == (3, H, W)
    detached = r3dgs_render.render(view, pc, PIPE, bg, distortion=NF, aux=("depth",), **options())
    assert not detached["depth"].requires_grad and detached["distortion"].requires_grad
    # the refusals
    with pytest.raises(ValueError):
        r3dgs_render.render(view, pc, PIPE, bg, distortion=(1.0, 0.5), **options())
    moving = scene_view(cam, H, W)
    moving.world_view_transform = moving.world_view_transform.clone().requires_grad_(True)
    with pytest.raises(ValueError, match="camera"):
        r3dgs_render.render(moving, pc, PIPE, bg, distortion=True, **options())


def test_behind_the_anti_aliasing_filters(C_):
    """render(distortion, antialiasing=True, filter_3d=f) equals a plain render of the filtered model."""
    import r3dgs_mip
    import r3dgs_render
    kw = ar.SCENE_A
    cam, g, _ = ar.make_scene(kw)
    H, W = kw["H"], kw["W"]
    pc, view, bg = Model(g), scene_view(cam, H, W), dev(BG)
    f = torch.full((kw["P"], 1), 0.01, device="cuda")
    out = r3dgs_render.render(view, pc, PIPE, bg, distortion=NF, antialiasing=True, filter_3d=f)
    filtered = r3dgs_render._antialiased_model(view, pc, PIPE, bg, 1.0, True, f)
    want = r3dgs_render.render(view, filtered, PIPE, bg, distortion=NF)
    assert torch.equal(out["distortion"], want["distortion"]) and torch.equal(out["render"], want["render"])
    assert float(out["distortion"].detach().max()) > 0
    out["distortion"].sum().backward()
    assert float(pc._scaling.grad.abs().max()) > 0 and float(pc._opacity.grad.abs().max()) > 0
    del r3dgs_mip


def test_quantised_and_empty_models_through_render(C_):
    import copy
    import r3dgs_render
    from tests import test_quantised_gpu as tq
    qm = copy.copy(tq.model("37-0-150-70")[0])
    c = tq.camera("131x77")
    qview = NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm, full_proj_transform=c.pm,
               camera_center=c.cp)
    out = r3dgs_render.render(qview, qm, PIPE, c.bg, distortion=True)
    fout = tq.quantised_forward(C_, qm, c)
    assert not out["distortion"].requires_grad
    assert torch.equal(out["distortion"], C_.distortion_map(qm.P, fout[0], c.H, c.W, fout[3], fout[4], fout[5]))
    qm.requires_grad_(True)
    with pytest.raises(ValueError, match="QuantisedModel"):
        r3dgs_render.render(qview, qm, PIPE, c.bg, distortion=True)
    cam, g, _ = ar.make_scene(dict(ar.SCENE_A, P=8))
    pc = Model({k: (v[:0] if hasattr(v, "shape") else v) for k, v in g.items()})
    out = r3dgs_render.render(scene_view(cam, 40, 56), pc, PIPE, dev(BG), distortion=True)
    assert out["distortion"].shape == (1, 40, 56) and not out["distortion"].any()
    out["distortion"].sum().backward()
