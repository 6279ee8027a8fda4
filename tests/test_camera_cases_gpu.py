"""GPU parity tests (-m gpu) at the cameras of tests/camera_cases.py: fx != fy, portrait, view rotations up to pi, a camera
centre 6 units from the origin.  Every other camera of the suite comes from synth_scene.make_camera: one focal length,
landscape, at most 0.1 rad per axis -- exchanging x and y in focal_x / focal_y, in the Jacobian's rows or in the clamp
limits of any kernel would pass there.

Nothing here has a bar of its own: the helpers and the bars are those of tests/test_gpu_parity.py (check_forward,
check_backward, mask_ambiguous: integers bit for bit, colour 1e-5, gradients 1e-4 against the fp32 oracle and the double
evaluation), tests/test_params_gpu.py and tests/test_quantised_gpu.py (bit for bit), tests/test_colour_variance.py (1e-5 away
from threshold-ambiguous pixels) and tests/test_reduction_ops.py (1e-5).  One cloud per camera (P = 3000, mixed degrees,
scale 0.05, seed 30) and one oracle evaluation of it, shared by the tests.

Threshold-ambiguous pixels the oracle flags at these clouds (gate 0.1 %, tests/test_gpu_parity.AMBIG_MAX_FRACTION; the
oracle alone, on the CPU): aniso 203x117 0.0042 % (1 pixel), portrait_far 117x203 0.0042 % (1), roll90_wide_clamp 203x117
0.0126 % (3), behind_tele 197x115 0.0221 % (5).  Seeds 30 .. 37 give 0 .. 0.093 %; the clamp camera has 9.6 % of its visible
Gaussians past the EWA clamp (|t.x / t.z| > 1.3 tanfovx or |t.y / t.z| > 1.3 tanfovy)."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import synth_scene as ss
from oracle import oracle as orc
from oracle import reduction_ops as ro
from tests import camera_cases as cc
from tests import quant_ref as qr
from tests import test_gpu_parity as gp
from tests import test_params_gpu as tp
from tests import test_quantised_gpu as tq
from tests.test_colour_variance import check_gpu_against_oracle
from tests.test_gpu_parity import (AMBIG_REL, check_backward, check_forward, hip_backward, hip_forward, mask_ambiguous,
                                   oracle_backward, oracle_forward)

pytestmark = pytest.mark.gpu

P, SEED, LAM = 3000, 30, 0.1
BG = np.array([0.1, 0.4, 0.9], np.float32)
CLAMP, FAR, BEHIND = "roll90_wide_clamp", "portrait_far", "behind_tele"


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


_cases = {}


def case(name):
    """The camera, its cloud, the oracle's forward of it, the masked upstream gradient and both oracle backwards: computed
    once, read by every test."""
    if name not in _cases:
        cam, g = cc.cloud(name, "gpu", P, SEED, "mixed", scale_mu=0.05)
        W, H = cc.CAMERAS[name]["gpu"][:2]
        ref = oracle_forward(BG, g, cam, H, W)
        dl = mask_ambiguous(ss.upstream_grad(W, H, seed=2) * (W * H), ref)
        gr, gr64 = oracle_backward(ref, dl, LAM)
        _cases[name] = NS(name=name, cam=cam, g=g, W=W, H=H, ref=ref, dl=dl, gr=gr, gr64=gr64, vis=ref["radii"] > 0)
    return _cases[name]


def renders_something(c, fout):
    assert fout[0].pairs > 0 and int(c.vis.sum()) > P // 4, "the case must render something"
    if c.name == CLAMP:
        f = cc.clamped_fraction(c.g, c.cam, c.vis)
        assert f >= 0.05, f"only {f:.3f} of the visible Gaussians are past the EWA clamp"


@pytest.mark.parametrize("name", list(cc.CAMERAS))
def test_dense_path_default_mode(C_, name):
    """(a) forward and backward of the library's default configuration, sparsity term on, against the fp32 oracle and the
    double evaluation."""
    c = case(name)
    fargs, fout = hip_forward(C_, BG, c.g, c.cam, c.H, c.W)
    renders_something(c, fout)
    check_forward(C_, fout, c.ref, c.H, c.W, P)
    bout = hip_backward(C_, fargs, fout, c.dl, LAM)
    check_backward(bout, c.gr, c.ref["state"], 16, gr64=c.gr64, tag=f" {{{name}}}")


@pytest.mark.parametrize("name", [FAR, CLAMP])
def test_reference_identical_configuration(C_, name):
    """(b) the reference's squares, the reference's fp32 covariance chain, the exact-size path: every exported integer list
    bit for bit, all nine gradient tensors through the reference-mode check (the chain's arithmetic bit for bit)."""
    c = case(name)
    was_rects, was_chain = C_.set_tight_rects(False), C_.set_f64_chain(False)
    try:
        assert not C_.tight_rects() and not C_.f64_chain()
        fargs, fout = hip_forward(C_, BG, c.g, c.cam, c.H, c.W, exact=True)
        assert fout[0].ticket == 0 and fout[0].pairs == int(fout[0]) == c.ref["num_rendered"]
        renders_something(c, fout)
        check_forward(C_, fout, c.ref, c.H, c.W, P)
        bout = hip_backward(C_, fargs, fout, c.dl, LAM)
        check_backward(bout, c.gr, c.ref["state"], 16, gr64=c.gr64, chain="f32", tag=f" {{{name}, reference mode}}", lam=LAM)
    finally:
        C_.set_tight_rects(was_rects)
        C_.set_f64_chain(was_chain)


def test_raw_parameter_pass_equals_the_existing_path(C_):
    """(c) rasterize_gaussian_params (activations fused into the per-Gaussian kernels) against the existing path on the
    activated values, portrait far-rotated camera: forward and the exported lists bit for bit, on the exact and on the
    reserved path; the gradients bit for bit (scaling / rotation through the host restatement of param_math.h)."""
    c = case(FAR)
    g, cam = c.g, c.cam
    rng = np.random.default_rng(5)
    rot_raw = (g["rotations"] * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)   # unnormalised, as a trained model's
    d = tp._dev
    s = dict(W=c.W, H=c.H, P=P, cam=cam, xyz=d(g["means3D"]), dc=d(g["sh"][:, :1]), rest=d(g["sh"][:, 1:]),
             opacity=d(g["opacity"]), scaling=d(np.log(g["scales"]).astype(np.float32)), rotation=d(rot_raw),
             degrees=d(g["degrees"]), bg=d(BG), vm=d(cam.world_view_transform), pm=d(cam.full_proj_transform),
             cp=d(cam.camera_center), dL=d(c.dl))
    act = C_.activate_params(s["scaling"], s["rotation"])
    sh = torch.cat((s["dc"], s["rest"]), dim=1)
    pairs = tp.existing_forward(C_, s, act, sh, True, None)[0].pairs
    for exact, reserve in ((True, None), (False, int(pairs * 1.25) + 4096)):
        out_e = tp.existing_forward(C_, s, act, sh, exact, reserve)
        out_f = tp.fused_forward(C_, s, exact, reserve)
        assert int(out_f[0]) == int(out_e[0]) and out_f[0].pairs == out_e[0].pairs == pairs > 0
        assert not out_f[0].truncated and not out_e[0].truncated
        assert int((out_e[2] > 0).sum()) > P // 4
        assert torch.equal(out_f[1], out_e[1]) and torch.equal(out_f[2], out_e[2])
        ex_e = C_.export_binning(P, out_e[0], c.H, c.W, out_e[3], out_e[4], out_e[5])
        ex_f = C_.export_binning(P, out_f[0], c.H, c.W, out_f[3], out_f[4], out_f[5])
        for k in ex_e:
            assert torch.equal(ex_e[k], ex_f[k]), k
        ge = tp.existing_backward(C_, s, act, sh, out_e, LAM)   # m2d, colors, opacity, m3d, cov3D, sh, scales, rotations
        gf = tp.fused_backward(C_, s, out_f, LAM)               # m2d, opacity, xyz, dc, rest, scaling, rotation
        assert tp.bits_equal(gf[0], ge[0]) and tp.bits_equal(gf[1], ge[2]) and tp.bits_equal(gf[2], ge[3])
        assert tp.bits_equal(gf[3], ge[5][:, :1].contiguous()) and tp.bits_equal(gf[4], ge[5][:, 1:].contiguous())
        want_sc, want_rot = tp.host_activation_backward(s, act, ge[6], ge[7])
        assert tp.bits_equal(gf[5], want_sc) and tp.bits_equal(gf[6], want_rot)
        assert gf[2].abs().max() > 0 and gf[4].abs().max() > 0 and gf[5].abs().max() > 0 and gf[6].abs().max() > 0


def test_ragged_inference_forward_reserved_equals_exact_equals_dense(C_):
    """(c) rasterize_gaussians_variableSH_bands over the degree-sorted ragged SH store, portrait far-rotated camera: the
    reserved path == the exact-size path == the dense training-path forward, bit for bit."""
    c = case(FAR)
    g, flat, per_band, cumsum, coeffs = gp.ragged_inputs(c.g)
    assert (per_band > 0).all()
    _, dense = hip_forward(C_, BG, g, c.cam, c.H, c.W, exact=True)
    assert dense[0].pairs > 0 and int((dense[2] > 0).sum()) > P // 4
    exd = C_.export_binning(P, dense[0], c.H, c.W, dense[3], dense[4], dense[5])
    rex = gp.hip_forward_ragged(C_, BG, g, flat, per_band, cumsum, coeffs, c.cam, c.H, c.W, exact=True)
    assert rex[0].ticket == 0
    outs = [rex] + [gp.hip_forward_ragged(C_, BG, g, flat, per_band, cumsum, coeffs, c.cam, c.H, c.W) for _ in range(3)]
    assert sum(1 for o in outs if o[0].ticket) >= 2          # the reserved path (and its graph replay) was taken
    for o in outs:
        assert int(o[0]) == int(dense[0]) and o[0].pairs == dense[0].pairs
        assert torch.equal(o[1], dense[1]) and torch.equal(o[2], dense[2])
        ex = C_.export_binning(P, o[0], c.H, c.W, o[3], o[4], o[5])
        for k in ("keys", "point_list", "ranges", "n_contrib", "final_T", "tiles_touched"):
            assert torch.equal(ex[k], exd[k]), k


def test_quantised_forward_equals_the_ragged_forward_of_the_decoded_model(C_):
    """(c) the codebook-indexed forward, portrait far-rotated camera: the 63-65-1-130 model of tests/test_quantised_gpu.py,
    its half positions carried in front of this camera, against the ragged forward of the decoded model -- bit for bit on
    the exact and on the reserved path."""
    cam = cc.camera(FAR, "gpu")
    W, H = cc.CAMERAS[FAR]["gpu"][:2]
    m = qr.make_model((63, 65, 1, 130), seed=11, half_xyz=True, half_centres=True, centre=(0.0, 0.0, 4.0), spread=0.8)
    m["xyz"] = cc.place_in_view(dict(means3D=m["xyz"].astype(np.float32)), cam)["means3D"].astype(np.float16)
    qm = tq.device_model(m)
    d = tq._dev
    c = NS(W=W, H=H, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, vm=d(cam.world_view_transform), pm=d(cam.full_proj_transform),
           cp=d(cam.camera_center), bg=d(BG))
    inputs = tq.ragged_inputs(C_, qm)
    for scale in (1.0, 0.5):
        want = tq.ragged_forward(C_, qm, inputs, c, scale)
        got = tq.quantised_forward(C_, qm, c, scale)
        tq.assert_same_pass(C_, qm.P, c, got, want, (FAR, scale, "exact"))
        assert want[0].pairs > 0 and (want[2] > 0).sum() > qm.P // 4, "the case must render something"
        reserve = int(want[0].pairs * 1.25) + 4096
        want_r = tq.ragged_forward(C_, qm, inputs, c, scale, exact=False, reserve=reserve)
        got_r = tq.quantised_forward(C_, qm, c, scale, exact=False, reserve=reserve)
        assert got_r[0].ticket > 0, "the reserved path was not taken"
        tq.assert_same_pass(C_, qm.P, c, got_r, want_r, (FAR, scale, "reserved"))
        assert torch.equal(got_r[1], got[1]) and torch.equal(got_r[2], got[2])


def near_ambiguous(ref):
    """Gaussians that can be blended into a threshold-ambiguous pixel.  alpha >= 1/255 with an opacity below 1 needs
    d' Sigma^-1 d <= 2 ln 255 = 11.08, so |d| <= 3.33 sqrt(lambda_max) <= 1.11 radius (radius = ceil(3 sqrt(lambda_max))):
    every Gaussian whose centre is within 1.11 radius + 1 of such a pixel in x and in y.  A decision taken the other way at
    that pixel changes the counters of these Gaussians and of no other."""
    xy, rad = ref["state"]["xy"], ref["radii"].astype(np.float32)
    near = np.zeros(len(rad), bool)
    ys, xs = np.nonzero(ref["ambig"])
    for x, y in zip(xs, ys):
        near |= (rad > 0) & (np.abs(xy[:, 0] - x) <= 1.11 * rad + 1) & (np.abs(xy[:, 1] - y) <= 1.11 * rad + 1)
    return near


@pytest.mark.parametrize("name", [BEHIND, CLAMP])
def test_mark_visible_and_counter_mode(C_, name):
    """(d) markVisible against the oracle's; counter mode (calculate_mean_transmittance) against the oracle's: touched
    pixels equal and the summed transmittance within 1e-5 for every Gaussian that cannot reach a threshold-ambiguous pixel
    (tests/test_colour_variance.py's bar for the same sums), tests/test_gpu_parity.py's bars on all of them."""
    c = case(name)
    g, cam = c.g, c.cam
    want_vis = orc.mark_visible(g["means3D"], cam.world_view_transform)
    got_vis = C_.mark_visible(gp.dev(g["means3D"]), gp.dev(cam.world_view_transform), gp.dev(cam.full_proj_transform))
    np.testing.assert_array_equal(got_vis.cpu().numpy(), want_vis)
    assert want_vis.sum() > P // 4 and (~want_vis).sum() > 0 and want_vis[c.vis].all()
    refc = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                       cam.full_proj_transform, cam.tanfovx, cam.tanfovy, c.H, c.W, g["sh"], g["degrees"], cam.camera_center,
                       counter_mode=True, want_ambig=True, ambig_rel=AMBIG_REL)
    np.testing.assert_array_equal(refc["ambig"], c.ref["ambig"])
    fargs, _ = hip_forward(C_, BG, g, cam, c.H, c.W)
    outc = C_.rasterize_gaussians_counters(*fargs)
    assert torch.equal(outc[2].cpu(), torch.from_numpy(c.ref["radii"]))
    touched, transm = outc[-2].cpu().numpy(), outc[-1].cpu().numpy()
    namb = int(refc["ambig"].sum())
    clean = ~near_ambiguous(refc)
    seen = refc["touched_pixels"] > 0
    assert seen.sum() > P // 4 and (clean & seen).sum() >= 0.5 * seen.sum(), ((clean & seen).sum(), seen.sum())
    np.testing.assert_array_equal(touched[clean], refc["touched_pixels"][clean])
    np.testing.assert_allclose(transm[clean], refc["transmittance"][clean], rtol=1e-5, atol=1e-6)
    err = np.abs(transm[clean & seen] - refc["transmittance"][clean & seen]) / refc["transmittance"][clean & seen]
    gp.achieved[f"[counter mode vs oracle] summed transmittance (rel) {{{name}}}"] = [
        float(err.max()), 0.0, f"test_mark_visible_and_counter_mode[{name}]"]
    assert np.abs(touched - refc["touched_pixels"]).sum() <= 2 * namb
    np.testing.assert_allclose(transm, refc["transmittance"], rtol=1e-4, atol=1e-3 + namb)


def four_camera_scene():
    """One quarter of the Gaussians in front of each of the four cameras, and the four cameras' arrays: image sizes, fields
    of view, view and projection matrices differ per camera."""
    names = list(cc.CAMERAS)
    cams = [cc.camera(n, "gpu") for n in names]
    parts = [cc.cloud(n, "gpu", P // 4, SEED + 1 + i, "mixed", scale_mu=0.05)[1] for i, n in enumerate(names)]
    g = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}
    return cams, g


def test_colour_variance_over_the_four_cameras(C_):
    """(e) calculate_colours_variance over a camera list made of the four cameras (per-camera H, W, tan(fov / 2)) against
    the oracle, at tests/test_colour_variance.py's bars."""
    cams, g = four_camera_scene()
    a = dict(cam_positions=np.stack([c.camera_center for c in cams]), means3D=g["means3D"], opacity=g["opacity"],
             scales=g["scales"], rotations=g["rotations"],
             cam_viewmatrices=np.stack([c.world_view_transform for c in cams]),
             cam_projmatrices=np.stack([c.full_proj_transform for c in cams]),
             tan_fovxs=np.array([c.tanfovx for c in cams], np.float32),
             tan_fovys=np.array([c.tanfovy for c in cams], np.float32),
             image_height=np.array([c.image_height for c in cams], np.int32),
             image_width=np.array([c.image_width for c in cams], np.int32), sh=g["sh"], degrees=g["degrees"], max_sh_deg=3)
    seen_by = np.zeros(len(g["means3D"]), np.int64)
    for i, c in enumerate(cams):
        o = orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, c.world_view_transform,
                        c.full_proj_transform, float(a["tan_fovxs"][i]), float(a["tan_fovys"][i]), c.image_height,
                        c.image_width, g["sh"], g["degrees"], c.camera_center, geometry_only=True)
        assert (o["radii"] > 0).sum() > P // 8, "every camera must see its part of the cloud"
        seen_by += o["radii"] > 0
    assert (seen_by >= 2).sum() > P // 8, "a variance needs Gaussians that several cameras see"
    check_gpu_against_oracle(a)


def test_minimum_projected_pixel_size_over_the_four_cameras(C_):
    """(e) find_minimum_projected_pixel_size with the four cameras' matrices and per-camera H / W (portrait: the pixel is
    measured along y) against the oracle, at tests/test_reduction_ops.py's bars."""
    cams, g = four_camera_scene()
    w2ndc = np.stack([c.full_proj_transform for c in cams]).astype(np.float32)
    w2ndc_inv = np.stack([np.linalg.inv(c.full_proj_transform.astype(np.float64)) for c in cams]).astype(np.float32)
    Hs = np.array([c.image_height for c in cams], np.int32)
    Ws = np.array([c.image_width for c in cams], np.int32)
    want, ambig = ro.min_pixel_size(w2ndc, w2ndc_inv, g["means3D"], Hs, Ws, want_ambig=True)
    got = C_.find_minimum_projected_pixel_size(gp.dev(w2ndc), gp.dev(w2ndc_inv), gp.dev(g["means3D"]), gp.dev(Hs),
                                               gp.dev(Ws)).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    ok = ~ambig
    assert ok.mean() > 0.95 and (want[ok] != 10000).mean() > 0.5 and (want[ok] == 10000).any()
    assert np.array_equal(got[ok] == 10000, want[ok] == 10000)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5)
    # each camera on its own as well: the minimum over the list must not hide one camera's value behind another's
    for i in range(len(cams)):
        want_i, ambig_i = ro.min_pixel_size(w2ndc[i:i + 1], w2ndc_inv[i:i + 1], g["means3D"], Hs[i:i + 1], Ws[i:i + 1],
                                            want_ambig=True)
        got_i = C_.find_minimum_projected_pixel_size(gp.dev(w2ndc[i:i + 1]), gp.dev(w2ndc_inv[i:i + 1]), gp.dev(g["means3D"]),
                                                     gp.dev(Hs[i:i + 1]), gp.dev(Ws[i:i + 1])).cpu().numpy()
        ok = ~ambig_i
        assert (want_i[ok] != 10000).sum() > P // 8
        assert np.array_equal(got_i[ok] == 10000, want_i[ok] == 10000)
        np.testing.assert_allclose(got_i[ok], want_i[ok], rtol=1e-5)


def test_zz_report_camera_case_distances(C_):
    """Not a check of its own: prints the distances the comparisons of this module reached, per camera (run with -s)."""
    tags = tuple("{" + n for n in cc.CAMERAS)
    for k in sorted(gp.achieved):
        if any(t in k for t in tags):
            print(f"  {k:<70s} max-normalised err {gp.achieved[k][0]:.2e}   elements outside the per-element bar "
                  f"{gp.achieved[k][1]:.2e}")
    print(f"threshold-ambiguous pixels masked per test (gate {100.0 * gp.AMBIG_MAX_FRACTION:.2f} %):")
    me = os.path.basename(__file__)[:-3]
    for k in sorted(gp.ambig_seen):
        if any(n in k for n in cc.CAMERAS) or me in k:
            print(f"  {k:<70s} {100.0 * gp.ambig_seen[k]:.4f} %")
