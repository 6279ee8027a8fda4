"""GPU tests (-m gpu) of the quantised forward: r3dgs_quantised_forward* / r3dgs_quantised_decode,
diff_gaussian_rasterization._C.rasterize_gaussians_quantised, r3dgs_quantised.QuantisedModel, r3dgs_render.render.

A codebook lookup copies a float and every half is a float exactly, so there is no tolerance anywhere in this file: the
quantised forward is held, bit for bit, to the EXISTING ragged inference forward fed what the quantised kernels compute
internally -- decode() (the same quant_math.h functions), _C.activate_params (the same param_math.h functions), and the
decoded SH rows packed into the fp32 ragged buffer -- in image, radii, num_rendered, pair count and the exported binning
(sorted keys, point list, tile ranges, n_contrib, final transmittance, tiles touched)."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import quant_ref as qr

pytestmark = pytest.mark.gpu
EMPTY = torch.Tensor([])
IMAGES = {"80x48": (80, 48, 60.0, 2), "131x77": (131, 77, 95.0, 4)}   # 5 x 3 whole tiles; partial tiles (W, H, focal, camera seed)
MODELS = {"-".join(map(str, c)): dict(counts=c) for c in qr.MIXES}
MODELS["P1"] = dict(counts=(0, 0, 1, 0), spread=0.0)
MODELS["behind"] = dict(counts=(20, 10, 30, 40), centre=(0.0, 0.0, -5.0), spread=0.5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_model(m):
    from r3dgs_quantised import QuantisedModel
    return QuantisedModel(_dev(m["xyz"]), _dev(m["geom_ids"]), _dev(m["sh_ids"]), _dev(m["codebooks"]), m["counts"])


_models = {}


def model(name, half=True):
    """(QuantisedModel on the device, its numpy arrays); the cloud sits 4 units in front of the cameras."""
    key = (name, half)
    if key not in _models:
        kw = dict(MODELS[name])
        kw.setdefault("centre", (0.0, 0.0, 4.0))
        kw.setdefault("spread", 0.8)
        m = qr.make_model(kw.pop("counts"), seed=len(name), half_xyz=half, half_centres=half, **kw)
        _models[key] = (device_model(m), m)
    return _models[key]


def camera(image, T=None):
    W, H, f, seed = IMAGES[image]
    cam = ss.make_camera(W, H, f, seed) if T is None else ss.Camera(W, H, f, f, None, T)
    return NS(W=W, H=H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, vm=_dev(cam.world_view_transform),
              pm=_dev(cam.full_proj_transform), cp=_dev(cam.camera_center), bg=_dev(np.array([0.1, 0.2, 0.3], np.float32)),
              FoVx=cam.FoVx, FoVy=cam.FoVy)


def quantised_forward(_C, qm, c, scale=1.0, exact=True, reserve=None, counters=None):
    return _C.rasterize_gaussians_quantised(c.bg, qm.xyz, qm.geom_ids, qm.sh_ids, qm.codebooks, scale, c.vm, c.pm, c.tanfovx,
                                            c.tanfovy, c.H, c.W, qm.per_band, qm.cumsum, qm.coeffs, c.cp, False, False,
                                            counters=counters, exact=exact, _reserve=reserve)


def ragged_inputs(_C, qm):
    """What the existing ragged inference forward takes for this model: decoded positions and opacity logits, activated
    scales and rotations, the stored SH coefficients of every Gaussian packed by degree."""
    d = qm.decode()
    scales, rotations = _C.activate_params(d["_scaling"], d["_rotation"])
    full = torch.cat((d["_features_dc"], d["_features_rest"]), dim=1)   # [P,16,3]
    rows, first = [], 0
    for deg, n in enumerate(qm.per_band_count):
        rows.append(full[first:first + n, :(deg + 1) ** 2].reshape(-1))
        first += n
    return d, scales, rotations, torch.cat(rows).contiguous()


def ragged_forward(_C, qm, inputs, c, scale=1.0, exact=True, reserve=None, counters=None):
    d, scales, rotations, sh = inputs
    with torch.no_grad():
        return _C._forward_common((qm.coeffs, qm.per_band, qm.cumsum), c.bg, d["_xyz"], EMPTY, d["_opacity"], scales, rotations,
                                  scale, EMPTY, c.vm, c.pm, c.tanfovx, c.tanfovy, c.H, c.W, sh, d["_degrees"], c.cp, False,
                                  False, counters=counters, exact=exact, _reserve=reserve)


def assert_same_pass(_C, P, c, got, want, what):
    assert int(got[0]) == int(want[0]) and got[0].pairs == want[0].pairs, what
    assert not got[0].truncated and not want[0].truncated, what
    assert torch.equal(got[1], want[1]), (what, "image")
    assert torch.equal(got[2], want[2]), (what, "radii")
    if want[0].pairs > 0:
        eg = _C.export_binning(P, got[0], c.H, c.W, got[3], got[4], got[5])
        ew = _C.export_binning(P, want[0], c.H, c.W, want[3], want[4], want[5])
        assert set(eg) >= {"keys", "point_list", "ranges", "final_T"}
        for k in ew:
            assert torch.equal(eg[k], ew[k]), (what, k)


@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("name", list(MODELS))
def test_quantised_equals_the_ragged_forward_of_the_decoded_model(name, image):
    from diff_gaussian_rasterization import _C
    qm, _ = model(name)
    c = camera(image)
    inputs = ragged_inputs(_C, qm)
    for scale in (1.0, 0.5):
        want = ragged_forward(_C, qm, inputs, c, scale)
        got = quantised_forward(_C, qm, c, scale)
        assert_same_pass(_C, qm.P, c, got, want, (name, image, scale, "exact"))
        if name == "behind":
            assert int(want[0]) == 0 and not want[2].any() and torch.equal(got[1], c.bg[:, None, None].expand(3, c.H, c.W))
        elif name != "P1":
            assert want[0].pairs > 0 and (want[2] > 0).sum() > qm.P // 4, "the case must render something"
        reserve = int(want[0].pairs * 1.25) + 4096   # one reservation for both sides, with room to spare
        want_r = ragged_forward(_C, qm, inputs, c, scale, exact=False, reserve=reserve)
        got_r = quantised_forward(_C, qm, c, scale, exact=False, reserve=reserve)
        assert got_r[0].ticket > 0, "the reserved path was not taken"
        assert_same_pass(_C, qm.P, c, got_r, want_r, (name, image, scale, "reserved"))
        assert torch.equal(got_r[1], got[1]) and torch.equal(got_r[2], got[2])


def counter_passes(_C, qm, c):
    """Counter mode (calculate_mean_transmittance) through the ragged fp32 path and through the quantised path."""
    inputs = ragged_inputs(_C, qm)
    outs = []
    for fwd, args in ((ragged_forward, (_C, qm, inputs, c)), (quantised_forward, (_C, qm, c))):
        touched = torch.zeros(qm.P, dtype=torch.int32, device="cuda")
        transm = torch.zeros(qm.P, dtype=torch.float32, device="cuda")
        out = fwd(*args, counters=(touched, transm))
        outs.append((out, touched, transm))
    return outs


def transmittance_rounding(c, sums):
    """How far two runs' out_transmittance sums may lie apart (test_counter_mode derives it): n positive addends summed in
    two orders differ by at most 2 (n-1) 2^-24 of the sum, n <= the image's 8x8 regions."""
    regions = ((c.W + 7) // 8) * ((c.H + 7) // 8)
    return 2 * (regions - 1) * 2.0 ** -24 * sums


@pytest.mark.parametrize("image", list(IMAGES))
def test_counter_mode(image):
    """A model whose Gaussians spread over many tiles.  The forward blend adds one float per (8x8-pixel region, Gaussian) to
    out_transmittance[id] with atomicAdd, in the order the workgroups get there, so a sum of three or more addends has last
    bits that depend on the run: the fp32 path does not reproduce its own (measured: 7..16 of these 259 sums differ by 1..2
    ulp between two runs of it).  Compared here: everything that is a function of the inputs (image, radii, the integer
    counters, which sums are non-zero) bit for bit, and the float sums to the rounding of a summation in any order --
    n positive addends summed in two orders differ by at most 2 (n-1) 2^-24 of the sum, n <= the image's 8x8 regions.
    test_counter_mode_transmittance_bits holds the sums themselves bit for bit."""
    from diff_gaussian_rasterization import _C
    qm, _ = model("63-65-1-130")
    c = camera(image)
    (want, t_w, m_w), (got, t_g, m_g) = counter_passes(_C, qm, c)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert t_w.sum() > 0 and torch.equal(t_g, t_w), "out_touched_pixels"
    assert (m_w > 0).any() and torch.equal(m_g > 0, m_w > 0)
    assert ((m_g - m_w).abs() <= transmittance_rounding(c, m_w)).all(), "out_transmittance"


def two_region_model(image):
    """The 63-65-1-130 mix as small splats laid out for `image`'s camera (R = I, T = 0) so that each one's sum in
    out_transmittance has at most two addends, which makes it independent of the order of the atomics (x + y = y + x exactly):
    every centre lies within half a pixel of the middle line of a row of 8x8 regions, anywhere along it, and no splat reaches
    further than `reach` < 4 pixels, so it stays inside its row and inside 8 consecutive columns -- two regions at most.
    reach: alpha >= 1/255 needs d' Sigma^-1 d <= 2 ln(255 opacity) < 2 ln 255, so |d| < sqrt(2 ln 255 lambda_max), and
    lambda_max <= (|J| s_max)^2 + 0.3 with |J| <= (f / z) sqrt(1 + (1.3 tanfovx)^2 + (1.3 tanfovy)^2); the scales are 0.1 to
    0.4 pixel at the nearest depth.  The layout is checked on the half positions the kernels read."""
    W, H, f, seed = IMAGES[image]
    m = qr.make_model((63, 65, 1, 130), seed=40 + seed, half_xyz=True, half_centres=True)
    rng = np.random.default_rng(seed)
    P = len(m["xyz"])
    m["codebooks"][17] = np.log(rng.uniform(0.1, 0.4, 256) * 3.5 / f).astype(np.float16).astype(np.float32)
    z = rng.uniform(3.5, 4.5, P)
    px = rng.uniform(2.0, W - 3.0, P)
    py = 8 * rng.integers(0, H // 8, P) + 3.5 + rng.uniform(-0.5, 0.5, P)
    m["xyz"] = np.stack(((px - (W - 1) / 2) * z / f, (py - (H - 1) / 2) * z / f, z), axis=1).astype(np.float16)
    x, y, z = m["xyz"].astype(np.float64).T
    px, py = f * x / z + (W - 1) / 2, f * y / z + (H - 1) / 2
    jac = f / z.min() * math.sqrt(1 + (1.3 * W / (2 * f)) ** 2 + (1.3 * H / (2 * f)) ** 2)
    lam = (jac * math.exp(float(m["codebooks"][17].max()))) ** 2 + 0.3
    reach = math.sqrt(2 * math.log(255.0) * lam)
    assert 2 * reach < 8 and (np.floor((py - reach) / 8) == np.floor((py + reach) / 8)).all(), (reach, "the layout")
    return device_model(m)


@pytest.mark.parametrize("image", list(IMAGES))
def test_counter_mode_transmittance_bits(image):
    """out_touched_pixels and out_transmittance bit for bit, on a model for which they are a function of the inputs
    (two_region_model): the fp32 path must reproduce its own, and the quantised path must equal it."""
    from diff_gaussian_rasterization import _C
    qm = two_region_model(image)
    c = camera(image, T=(0.0, 0.0, 0.0))
    (want, t_w, m_w), (got, t_g, m_g) = counter_passes(_C, qm, c)
    (_, t_a, m_a), _ = counter_passes(_C, qm, c)
    differ = (m_g.view(torch.int32) != m_w.view(torch.int32))
    print(f"out_transmittance: {int(differ.sum())} of {m_w.numel()} differ, max |diff| in ulp "
          f"{int((m_g.view(torch.int32) - m_w.view(torch.int32)).abs().max())}; mean T {float(m_w.sum() / t_w.sum()):.3f}")
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert (t_w > 0).sum() > qm.P // 2 and (m_w < 0.9 * t_w).any(), "the splats must show, and some behind others"
    assert torch.equal(t_a, t_w) and torch.equal(m_a.view(torch.int32), m_w.view(torch.int32)), "the fp32 path against itself"
    assert torch.equal(t_g, t_w), "out_touched_pixels"
    assert torch.equal(m_g.view(torch.int32), m_w.view(torch.int32)), "out_transmittance"


def test_against_the_dense_training_path_and_the_padding_does_not_leak():
    from diff_gaussian_rasterization import _C
    counts = (37, 13, 150, 0)   # no degree-3 Gaussian: nothing stores an id of features_rest_9..14
    m = qr.make_model(counts, seed=7, half_xyz=True, half_centres=True, centre=(0.0, 0.0, 4.0), spread=0.8)
    m["codebooks"][:16, 0] = 0.75   # centre 0 of every SH codebook: what the reference's loader pads with
    qm = device_model(m)
    c = camera("131x77")
    got = quantised_forward(_C, qm, c)
    d = qm.decode()
    above = torch.arange(1, 16, device="cuda")[None, :] >= ((d["_degrees"].long().reshape(-1) + 1) ** 2)[:, None]
    assert (d["_features_rest"][above] != 0).any(), "the decoded padding (centre 0 of each codebook) is not zero here"
    with torch.no_grad():
        dense = _C.rasterize_gaussian_params(c.bg, d["_xyz"], d["_features_dc"], d["_features_rest"], d["_degrees"], d["_opacity"],
                                             d["_scaling"], d["_rotation"], 1.0, c.vm, c.pm, c.tanfovx, c.tanfovy, c.H, c.W,
                                             c.cp, False, False, exact=True)
    assert (got[2] > 0).sum() > 50
    assert torch.equal(got[1], dense[1]) and torch.equal(got[2], dense[2])
    qm.codebooks[15, 0] = 1.0e6   # centre 0 of features_rest_14: only padding refers to it
    again = quantised_forward(_C, qm, c)
    assert torch.equal(again[1], got[1]) and torch.equal(again[2], got[2])


def test_graph_replay_reads_the_model_through_its_pointers():
    from diff_gaussian_rasterization import _C
    m = qr.make_model((40, 30, 50, 60), seed=21, centre=(0.0, 0.0, 4.0), spread=0.8)
    qm = device_model(m)
    c = camera("80x48")
    reserve = int(quantised_forward(_C, qm, c)[0].pairs * 1.25) + 4096
    stats = _C.pass_stats()
    first = quantised_forward(_C, qm, c, exact=False, reserve=reserve)
    image1, radii1 = first[1].clone(), first[2].clone()
    # the same tensors, new contents: more opaque and another colour
    qm.codebooks[16] += 1.5
    qm.codebooks[0] = qm.codebooks[0].flip(0) * 0.5 + 0.25
    second = quantised_forward(_C, qm, c, exact=False, reserve=reserve)
    after = _C.pass_stats()
    assert after["reserved_passes"] == stats["reserved_passes"] + 2 and after["redone_passes"] == stats["redone_passes"]
    fresh = quantised_forward(_C, device_model(qr.model_arrays(qm)), c)   # exact path, arrays of their own
    assert torch.equal(second[1], fresh[1]) and torch.equal(second[2], fresh[2])
    assert not torch.equal(second[1], image1) and torch.equal(second[2], radii1)


@pytest.mark.parametrize("half", [True, False])
def test_fixture_files_decode_and_render(half, golden_dir):
    """The files the reference's save_ply wrote: decode() on the device equals its load_ply bit for bit in all seven
    tensors, and the forward -- fp32 positions for quantised_P200.ply -- equals the ragged forward of the decoded model."""
    import os

    from diff_gaussian_rasterization import _C
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_half_P200.ply" if half else "quantised_P200.ply"), half)
    assert qm.device.type == "cuda" and qm.xyz.dtype == (torch.float16 if half else torch.float32)
    want = np.load(os.path.join(golden_dir, "quantised_P200_loaded.npz"))
    d = qm.decode()
    for k in qr.KEYS:
        w = want[("half" if half else "float") + k]
        g = d[k].cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(qr.bits(g), qr.bits(w)), k
    assert qm.nbytes == sum(t.numel() * t.element_size() for t in qm.arrays())
    inputs = ragged_inputs(_C, qm)
    for image in IMAGES:
        c = camera(image, T=(0.1, -0.05, 4.0))   # the file's cloud sits around the origin
        want_e = ragged_forward(_C, qm, inputs, c)
        got_e = quantised_forward(_C, qm, c)
        assert (want_e[2] > 0).sum() > 100
        assert_same_pass(_C, qm.P, c, got_e, want_e, (half, image, "exact"))
        reserve = int(want_e[0].pairs * 1.25) + 4096
        assert_same_pass(_C, qm.P, c, quantised_forward(_C, qm, c, exact=False, reserve=reserve),
                         ragged_forward(_C, qm, inputs, c, exact=False, reserve=reserve), (half, image, "reserved"))


def test_strict_redo_and_lossy_opt_out(golden_dir):
    """tests/test_train_loop_gpu.py's test of that name for the quantised forward, on quantised_P200.ply at 80x48, the
    smallest case of test_fixture_files_decode_and_render (more than 100 of its Gaussians show there, so R // 2 > 0): the
    same overflowing reservation through strict mode (default: result == exact path, one redo counted; counter mode not
    counted twice) and with strict mode off (farthest pairs dropped, pass flagged)."""
    import os

    from diff_gaussian_rasterization import _C
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    c = camera("80x48", T=(0.1, -0.05, 4.0))
    P = qm.P
    exact = quantised_forward(_C, qm, c)
    R = exact[0].pairs
    assert R >= 2
    s0 = _C.pass_stats()
    out = quantised_forward(_C, qm, c, exact=False, reserve=R // 2)            # strict (default)
    s1 = _C.pass_stats()
    assert s1["redone_passes"] == s0["redone_passes"] + 1
    assert not out[0].truncated and out[0].pairs == R and int(out[0]) == int(exact[0])
    assert torch.equal(out[1], exact[1]) and torch.equal(out[2], exact[2])
    # counter mode accumulates into its outputs: the redo must not count the truncated pass as well
    touched, transm = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(P, device="cuda")
    touched_x, transm_x = torch.zeros_like(touched), torch.zeros_like(transm)
    quantised_forward(_C, qm, c, counters=(touched_x, transm_x))
    quantised_forward(_C, qm, c, exact=False, reserve=R // 2, counters=(touched, transm))
    assert touched_x.sum() > 0 and torch.equal(touched, touched_x)
    assert torch.allclose(transm, transm_x, rtol=1e-5, atol=1e-4)   # float atomics: order-dependent low bits
    lossy = _C.rasterize_gaussians_quantised(c.bg, qm.xyz, qm.geom_ids, qm.sh_ids, qm.codebooks, 1.0, c.vm, c.pm, c.tanfovx,
                                             c.tanfovy, c.H, c.W, qm.per_band, qm.cumsum, qm.coeffs, c.cp, False, False,
                                             _reserve=R // 2, _strict_override=False)
    assert lossy[0].truncated and not torch.equal(lossy[1], exact[1])


class DecodedModel:
    """decode()'s tensors shaped like the reference's GaussianModel with variable_sh_bands: get_features is the list of
    per-degree tensors.  Its activations are this repository's (_C.activate_params)."""

    def __init__(self, _C, qm):
        d = qm.decode()
        for k, v in d.items():
            setattr(self, k, v)
        self.get_xyz, self.per_band_count = d["_xyz"], qm.per_band_count
        self.get_scaling, self.get_rotation = _C.activate_params(d["_scaling"], d["_rotation"])
        self.active_sh_degree = self.max_sh_degree = 3
        full = torch.cat((d["_features_dc"], d["_features_rest"]), dim=1)
        self.get_features, first = [], 0
        for deg, n in enumerate(qm.per_band_count):
            self.get_features.append(full[first:first + n, :(deg + 1) ** 2].contiguous())
            first += n


def test_render_accepts_a_quantised_model(monkeypatch):
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    qm, _ = model("37-0-150-70")
    c = camera("131x77")
    view = NS(image_height=c.H, image_width=c.W, FoVx=c.FoVx, FoVy=c.FoVy, world_view_transform=c.vm,
              full_proj_transform=c.pm, camera_center=c.cp)
    pipe = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    dm = DecodedModel(_C, qm)
    for scale in (1.0, 0.5):
        with torch.no_grad():
            want = r3dgs_render.render(view, dm, pipe, c.bg, scaling_modifier=scale, variable_sh_bands=True)
        got = r3dgs_render.render(view, qm, pipe, c.bg, scaling_modifier=scale)
        assert set(got) == set(want) and got["viewspace_points"] is None
        assert torch.equal(got["render"], want["render"]) and torch.equal(got["radii"], want["radii"])
        assert torch.equal(got["visibility_filter"], want["visibility_filter"]) and want["visibility_filter"].sum() > 50
    assert r3dgs_render.render(view, qm, pipe, c.bg, measure_fps=True)["FPS"] > 0
    for kw, pp, msg in ((dict(override_color=torch.zeros(qm.P, 3, device="cuda")), pipe, "override_color is not supported"),
                        ({}, NS(debug=False, compute_cov3D_python=True, convert_SHs_python=False), "compute_cov3D_python is not"),
                        ({}, NS(debug=False, compute_cov3D_python=False, convert_SHs_python=True), "convert_SHs_python is not")):
        with pytest.raises(ValueError, match=msg):
            r3dgs_render.render(view, qm, pp, c.bg, **kw)
    # an ordinary model takes the route it took before: the fused raw-parameter forward, and never the quantised entry
    from diff_gaussian_rasterization import GaussianRasterizationSettings, rasterize_gaussian_params
    monkeypatch.setattr(_C, "rasterize_gaussians_quantised", None)
    dense = r3dgs_render.render(view, dm, pipe, c.bg)
    rs = GaussianRasterizationSettings(c.H, c.W, c.tanfovx, c.tanfovy, c.bg, 1.0, c.vm, c.pm, 3, c.cp, False, False)
    image, radii = rasterize_gaussian_params(dm._xyz, torch.zeros_like(dm._xyz), dm._features_dc, dm._features_rest, dm._degrees,
                                             dm._opacity, dm._scaling, dm._rotation, rs, 0.0)
    assert torch.equal(dense["render"], image) and torch.equal(dense["radii"], radii) and dense["viewspace_points"] is not None
