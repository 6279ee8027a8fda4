"""GPU tests (-m gpu) of the per-Gaussian backward's load phase (csrc/preprocess_bwd.hip): every per-lane input is requested
before the first use and the tests that used to guard the loads -- the stamp test, `start + ntile <= num_pairs`,
`deg > 0 && ntile > 0`, `w0 == w1` -- are applied to the loaded values.  One scene of 1 037 Gaussians at 320 x 240 that
reaches every branch those selects replaced:
  * P = 1 000 + 37: a tail wave of 13 lanes (lanes i >= P issue no load);
  * Gaussians 128..255 behind the camera (two whole waves culled), 256..319 culled but one (a wave with one visible lane);
  * Gaussians 64..79 with an opacity below 1 / 255: visible, binned into no tile (ntile == 0);
  * Gaussians 400..402 over more than 128 tiles, 403..405 over more than 64: their pair runs span three / two 64-pair groups
    (w0 != w1, the wave_part walk -- the one dependent load left);
  * degrees mixed 0..3.
All nine gradient tensors are held to the two oracles with the helpers and the bars of tests/test_gpu_parity.py; library paths
that must agree (raw-parameter pass / existing pass on activated values, forward's direction derivatives / row-reading
backward) agree bit for bit.  Every test runs under a time limit of its own (a watchdog thread ends the process)."""
import faulthandler

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests.test_gpu_parity import (GRAD_REL, check_backward, dev, hip_backward, hip_forward, mask_ambiguous, oracle_backward,
                                   oracle_forward)

pytestmark = pytest.mark.gpu
W, H, P = 320, 240, 1037
TEST_TIME_LIMIT_S = 120
EMPTY = torch.Tensor([])


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TEST_TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def C_():
    from diff_gaussian_rasterization import _C
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _C


_cache = {}


def scene():
    """-> (cam, g, bg, ref, dl, dl2): the oracle's forward is computed once and shared."""
    if "scene" in _cache:
        return _cache["scene"]
    cam = ss.make_camera(W, H, 250.0, 3)
    g = ss.make_gaussians(P, cam, seed=21, degree_mode="mixed", scale_mu=0.03, behind_frac=0.0, zmin=2.0, zmax=8.0)
    m = g["means3D"]
    m[128:320, 2] = -1.0                    # behind the camera: culled
    m[300] = (0.3, -0.2, 4.0)               # ... but one lane of wave 4
    g["opacity"][64:80] = -8.0              # sigmoid(-8) < 1 / 255: no tile can hold a pixel it reaches
    m[64:80, :2] *= 0.5                     # (well inside the frustum)
    for k, (i, s_) in enumerate(((400, 0.8), (401, 0.7), (402, 0.9), (403, 0.42), (404, 0.4), (405, 0.44))):
        m[i] = (0.4 * (k % 3 - 1), 0.3 * (k // 3) - 0.15, 4.0 + 0.2 * k)
        g["scales"][i] = (s_, 0.9 * s_, 0.02)
        g["rotations"][i] = (1.0, 0.0, 0.0, 0.0)
        g["opacity"][i] = 1.5
    bg = np.array([0.1, 0.4, 0.9], np.float32)
    ref = oracle_forward(bg, g, cam, H, W)
    dl = mask_ambiguous(ss.upstream_grad(W, H, seed=2) * (W * H), ref)
    dl2 = mask_ambiguous(ss.upstream_grad(W, H, seed=9) * (W * H), ref)
    dl2[:, :, : W // 2] = 0.0               # second pass: the Gaussians of the left half now sum to exact zeros
    _cache["scene"] = (cam, g, bg, ref, dl, dl2)
    return _cache["scene"]


def oracle_grads(which, lam):
    key = ("grads", which, lam)
    if key not in _cache:
        _, _, _, ref, dl, dl2 = scene()
        _cache[key] = oracle_backward(ref, dl if which == 1 else dl2, lam)
    return _cache[key]


def test_scene_reaches_every_branch(C_):
    cam, g, bg, ref, dl, _ = scene()
    fargs, fout = hip_forward(C_, bg, g, cam, H, W, exact=True)
    radii = fout[2].cpu().numpy().reshape(-1)
    ex = C_.export_binning(P, fout[0], H, W, fout[3], fout[4], fout[5])
    tiles = ex["tiles_touched"].cpu().numpy().astype(np.int64).reshape(-1)
    assert P % 64 != 0 and P % 256 != 0
    assert (radii[128:256] == 0).all(), "two whole waves culled"
    assert (radii[256:320] > 0).sum() == 1 and radii[300] > 0, "a wave with one visible lane"
    assert ((radii[64:80] > 0) & (tiles[64:80] == 0)).sum() >= 8, "visible Gaussians binned into no tile"
    assert (tiles[400:403] > 128).all() and (tiles[403:406] > 64).all(), (tiles[400:406],)
    assert set(np.unique(g["degrees"][radii > 0])) == {0, 1, 2, 3}
    assert (radii[P - 13:] > 0).any(), "the tail wave has visible lanes"


@pytest.mark.parametrize("chain", ["f64", "f32"])
@pytest.mark.parametrize("lam", [0.0, 0.1])
def test_nine_gradients_against_the_oracles(C_, lam, chain):
    """lam = 0: the forward's direction derivatives (cached path); lam = 0.1: the row-reading path.  chain f32:
    set_f64_chain(False), the reference's arithmetic, held to the fp32 oracle at 1e-4 as the golden cases are."""
    cam, g, bg, ref, dl, _ = scene()
    gr, gr64 = oracle_grads(1, lam)
    was = C_.set_f64_chain(chain == "f64")
    try:
        for exact in (True, False):   # exact-size path, then whichever the library picks (reserved / graph)
            fargs, fout = hip_forward(C_, bg, g, cam, H, W, exact=exact)
            bout = hip_backward(C_, fargs, fout, dl, lam)
            if chain == "f64":
                check_backward(bout, gr, ref["state"], 16, gr64=gr64)
            else:
                check_backward(bout, gr, ref["state"], 16, gr64=gr64, chain="f32", chain_fp32_rel=GRAD_REL, lam=lam)
            if exact:
                first = bout
            else:
                for a, b in zip(first, bout):
                    assert torch.equal(a, b)
    finally:
        C_.set_f64_chain(was)
    assert float(bout[0][400:406].abs().max()) > 0, "the splats whose runs span several groups got their pieces"
    assert (bout[1][64:80] == 0).all() and (bout[0][64:80] == 0).all(), "binned into no tile: no colour, no 2D-stage gradient"


def test_second_backward_over_the_same_buffers_reads_stale_rows_as_zero(C_):
    """pair_reduce stores no row for a run whose nine sums are zero; the reader takes a row without this pass's stamp for
    zeros.  The second pass's upstream gradient vanishes on the left half of the image, so the rows the first pass left
    for the Gaussians there are stale and must not be read."""
    cam, g, bg, ref, dl, dl2 = scene()
    fargs, fout = hip_forward(C_, bg, g, cam, H, W)
    first = hip_backward(C_, fargs, fout, dl, 0.0)
    second = hip_backward(C_, fargs, fout, dl2, 0.0)
    gr, gr64 = oracle_grads(2, 0.0)
    check_backward(second, gr, ref["state"], 16, gr64=gr64)
    stale = (first[0].abs().sum(dim=1) > 0) & (second[0].abs().sum(dim=1) == 0) & (fout[2].reshape(-1) > 0)
    assert int(stale.sum()) >= 20, "the second pass must leave Gaussians without a row that the first pass wrote one for"
    want = torch.from_numpy(gr["dL_dmeans2D"]).cuda().reshape(P, -1)
    assert (want[stale].abs().sum(dim=1) == 0).all()
    again = hip_backward(C_, fargs, fout, dl, 0.0)   # and back: every row is this pass's again
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_precomputed_covariance(C_):
    cam, g, bg, ref, dl, _ = scene()
    cov = ref["state"]["cov3D"].copy()
    cov[(cov == 0).all(1)] = np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32)
    refc = oracle_forward(bg, g, cam, H, W, cov=cov, use_sr=False)
    dlc = mask_ambiguous(ss.upstream_grad(W, H, seed=2) * (W * H), refc)
    for lam in (0.0, 0.1):
        fargs, fout = hip_forward(C_, bg, g, cam, H, W, cov=cov, use_sr=False)
        bout = hip_backward(C_, fargs, fout, dlc, lam)
        gr, gr64 = oracle_backward(refc, dlc, lam)
        check_backward(bout, gr, refc["state"], 16, gr64=gr64)
        assert (bout[6] == 0).all() and (bout[7] == 0).all()


def _raw_scene():
    cam, g, bg, ref, dl, _ = scene()
    rng = np.random.default_rng(5)
    rot_raw = (g["rotations"] * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)   # unnormalised, as a trained model's
    return dict(cam=cam, bg=dev(bg), xyz=dev(g["means3D"]), dc=dev(g["sh"][:, :1]), rest=dev(g["sh"][:, 1:]),
                opacity=dev(g["opacity"]), scaling=dev(np.log(g["scales"]).astype(np.float32)), rotation=dev(rot_raw),
                degrees=dev(g["degrees"]), vm=dev(cam.world_view_transform), pm=dev(cam.full_proj_transform),
                cp=dev(cam.camera_center), dL=dev(dl))


@pytest.mark.parametrize("overflow", [False, True], ids=["fits", "reservation_overflows"])
@pytest.mark.parametrize("lam", [0.0, 0.1])
def test_raw_parameter_pass_equals_existing_pass_bit_for_bit(C_, lam, overflow):
    """rasterize_gaussian_params against rasterize_gaussians fed the activated values (tests/test_params_gpu.py), on this
    scene -- and on a pass whose pair reservation is half of what the pass wants (strict mode off, as
    tests/test_train_loop_gpu.py reaches it): the farthest pairs are dropped, and every Gaussian whose pairs did not all fit
    (`start + ntile > num_pairs`) gets exactly zero 2D-stage gradients on both paths."""
    from tests.test_params_gpu import bits_equal, host_activation_backward
    s = _raw_scene()
    c = s["cam"]
    act = C_.activate_params(s["scaling"], s["rotation"])
    sh = torch.cat((s["dc"], s["rest"]), dim=1)
    common = (1.0, EMPTY, s["vm"], s["pm"], c.tanfovx, c.tanfovy, H, W)
    exact_out = C_._forward_common(None, s["bg"], s["xyz"], EMPTY, s["opacity"], act[0], act[1], *common, sh, s["degrees"], s["cp"],
                                   False, False, exact=True)
    pairs = exact_out[0].pairs
    kw = dict(_reserve=pairs // 2, _strict_override=False) if overflow else dict(_reserve=int(pairs * 1.25) + 4096)
    out_e = C_._forward_common(None, s["bg"], s["xyz"], EMPTY, s["opacity"], act[0], act[1], *common, sh, s["degrees"], s["cp"],
                               False, False, **kw)
    out_f = C_.rasterize_gaussian_params(s["bg"], s["xyz"], s["dc"], s["rest"], s["degrees"], s["opacity"], s["scaling"],
                                         s["rotation"], 1.0, s["vm"], s["pm"], c.tanfovx, c.tanfovy, H, W, s["cp"], False, False,
                                         **kw)
    assert bool(out_e[0].truncated) == overflow and bool(out_f[0].truncated) == overflow
    assert torch.equal(out_f[1], out_e[1]) and torch.equal(out_f[2], out_e[2])

    def bwd_e(out):
        nr, _, radii, geom, binning, img = out
        return C_.rasterize_gaussians_backward(s["bg"], s["xyz"], radii, EMPTY, act[0], act[1], 1.0, EMPTY, s["vm"], s["pm"],
                                               c.tanfovx, c.tanfovy, s["dL"], sh, s["degrees"], s["cp"], geom, nr, binning, img,
                                               lam, False)
    ge = bwd_e(out_e)      # m2d, colors, opacity, m3d, cov3D, sh, scales, rotations
    nr, _, radii, geom, binning, img = out_f
    gf = C_.rasterize_gaussian_params_backward(s["bg"], s["xyz"], radii, s["dc"], s["rest"], s["degrees"], s["opacity"],
                                               s["scaling"], s["rotation"], 1.0, s["vm"], s["pm"], c.tanfovx, c.tanfovy, s["dL"],
                                               s["cp"], geom, nr, binning, img, lam, False)   # m2d, opacity, xyz, dc, rest, scaling, rot
    assert bits_equal(gf[0], ge[0]) and bits_equal(gf[1], ge[2]) and bits_equal(gf[2], ge[3])
    assert bits_equal(gf[3], ge[5][:, :1].contiguous()) and bits_equal(gf[4], ge[5][:, 1:].contiguous())
    want_sc, want_rot = host_activation_backward(s, act, ge[6], ge[7])
    assert bits_equal(gf[5], want_sc) and bits_equal(gf[6], want_rot)
    for t in ge + gf:
        assert torch.isfinite(t).all()
    if lam == 0.0:   # the forward's direction derivatives against the row-reading backward, on the same state
        was = C_.set_sh_cache(False)
        try:
            for a, b in zip(ge, bwd_e(out_e)):
                assert torch.equal(a, b)
        finally:
            C_.set_sh_cache(was)
    if overflow:
        full = bwd_e(exact_out)
        dropped = (full[0].abs().sum(dim=1) > 0) & (ge[0].abs().sum(dim=1) == 0)
        assert int(dropped.sum()) > 0, "no Gaussian lost its pairs: the reservation did not overflow"
        for t in (ge[0], ge[1], ge[2]):   # 2D-stage sums: zero, not partial
            assert (t[dropped] == 0).all()
