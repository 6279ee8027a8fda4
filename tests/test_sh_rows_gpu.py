"""GPU tests (-m gpu) of the SH-row staging shared by the forward's colour role, the per-Gaussian backward and the colour
variance step (csrc/sh_rows.h), at the smallest shapes where it can go wrong: every SH stride M that has its own path
(1: no rest span, 4 / 9: the general skew, 16: rows of 48) x a partial wave whose length is no multiple of 4, full waves
followed by a two-row wave, and a second forward workgroup.  The dense entry (activated tensors, one SH tensor) and the split
entry (raw parameters, features_dc / features_rest) share that code, so comparing them with each other cannot find a mistake
they share: both are held to the CPU oracle (oracle/oracle.py, any M), which knows nothing of waves or LDS."""
import math

import numpy as np
import pytest
import torch

import synth_scene as ss
from oracle import oracle as orc
from tests import test_gpu_parity as gp
from tests import test_params_gpu as pg
from tests.test_colour_variance import check_gpu_against_oracle

pytestmark = pytest.mark.gpu
W, H = 64, 48
SHAPES = [(P, M) for P in (61, 130, 259) for M in (1, 4, 9, 16)]


def host_scene(P, M):
    """Seeded Gaussians in front of a 64 x 48 camera, SH rows of M coefficients, degrees 0 .. what M allows in turn (so every
    wave mixes them), raw scaling / rotation as a model stores them and their float32 activations as the host computes them."""
    cam = ss.make_camera(W, H, 50.0, 2)
    g = ss.make_gaussians(P, cam, seed=100 + P, degree_mode="all3", scale_mu=0.05, behind_frac=0.1)
    g["sh"] = np.ascontiguousarray(g["sh"][:, :M])
    g["degrees"] = (np.arange(P) % math.isqrt(M)).astype(np.int32).reshape(P, 1)
    rng = np.random.default_rng(5)
    g["rotation_raw"] = (g["rotations"] * rng.uniform(0.3, 3.0, (P, 1))).astype(np.float32)   # unnormalised, as a trained model's
    g["scaling_raw"] = np.log(g["scales"]).astype(np.float32)
    return cam, g


_cases = {}


def case(P, M):
    """-> (s, g, ref): the device tensors in tests/test_params_gpu.py's form, the host arrays the oracle gets (the scales and
    rotations are the DEVICE's activations, so both entries and the oracle start from the same bits) and the oracle's forward.
    Built once per shape and left unchanged."""
    if (P, M) in _cases:
        return _cases[(P, M)]
    from diff_gaussian_rasterization import _C
    cam, g = host_scene(P, M)
    s = dict(W=W, H=H, P=P, cam=cam, xyz=pg._dev(g["means3D"]), dc=pg._dev(g["sh"][:, :1]), rest=pg._dev(g["sh"][:, 1:]),
             opacity=pg._dev(g["opacity"]), scaling=pg._dev(g["scaling_raw"]), rotation=pg._dev(g["rotation_raw"]),
             degrees=pg._dev(g["degrees"]), bg=pg._dev(np.array([0.1, 0.2, 0.3], np.float32)), vm=pg._dev(cam.world_view_transform),
             pm=pg._dev(cam.full_proj_transform), cp=pg._dev(cam.camera_center))
    act = _C.activate_params(s["scaling"], s["rotation"])
    g = dict(g, scales=act[0].cpu().numpy(), rotations=act[1].cpu().numpy())
    ref = gp.oracle_forward(np.array([0.1, 0.2, 0.3], np.float32), g, cam, H, W)
    dl = gp.mask_ambiguous(ss.upstream_grad(W, H, seed=1) * (W * H), ref)
    s.update(act=act, sh=torch.cat((s["dc"], s["rest"]), dim=1).contiguous(), dL=pg._dev(dl), dl_host=dl)
    _cases[(P, M)] = (s, g, ref)
    return _cases[(P, M)]


def assert_scene_exercises_the_paths(P, M, g, ref):
    vis = ref["radii"] > 0
    assert vis.any() and (~vis).any(), "the case needs visible and culled Gaussians"
    deg = g["degrees"].reshape(-1)
    for d in range(math.isqrt(M)):
        assert ((deg == d) & vis).any(), f"no visible Gaussian of degree {d}"
    for w0 in range(0, P, 64):   # every wave mixes the degrees and, but for a tail of a few rows, holds a visible Gaussian
        assert len(set(deg[w0:w0 + 64])) == min(math.isqrt(M), len(deg[w0:w0 + 64]))
    assert vis[P - P % 64:].any() or P % 64 == 0, "the tail wave has to stage its rows"


def dense_backward_into_nan(_C, s, out, lam):
    """The dense entry with every output in NaN-filled storage (the gradient arena hands the library its buffers)."""
    _C.set_gradient_arena(lambda name, shape: torch.full(shape, float("nan"), device="cuda"))
    try:
        return pg.existing_backward(_C, s, s["act"], s["sh"], out, lam)
    finally:
        _C.set_gradient_arena(None)


@pytest.mark.parametrize("P,M", SHAPES)
def test_staging_against_the_oracle_dense_and_split(P, M):
    from diff_gaussian_rasterization import _C
    s, g, ref = case(P, M)
    assert_scene_exercises_the_paths(P, M, g, ref)
    vis = torch.from_numpy(ref["radii"] > 0).cuda()
    above = torch.from_numpy(np.arange(M)[None, :] >= ((g["degrees"].reshape(-1).astype(np.int64) + 1) ** 2)[:, None]).cuda()
    # ---- forward: the dense entry against the oracle (test_golden_cases_forward_backward's checks), the split entry equal to it
    out_e = pg.existing_forward(_C, s, s["act"], s["sh"], True, None)
    out_f = pg.fused_forward(_C, s, True, None)
    gp.check_forward(_C, out_e, ref, H, W, P)
    assert int(out_f[0]) == int(out_e[0]) and out_f[0].pairs == out_e[0].pairs
    assert torch.equal(out_f[1], out_e[1]), "image"
    assert torch.equal(out_f[2], out_e[2]), "radii"
    # ---- backward: with the sparsity term (the rows are read), without it and the direction-derivative cache off (read
    # again), and with the cache on (not read: the rows the kernel writes are still all of dL_dsh)
    for lam, cache in ((0.1, True), (0.0, False), (0.0, True)):
        r32, r64 = gp.oracle_backward(ref, s["dl_host"], lam)
        was = _C.set_sh_cache(cache)
        try:
            ge = dense_backward_into_nan(_C, s, out_e, lam)   # m2d, colors, opacity, m3d, cov3D, sh, scales, rotations
            gf = pg.fused_backward(_C, s, out_f, lam)         # m2d, opacity, xyz, dc, rest, scaling, rotation
            gn = pg.fused_backward_into_nan(_C, s, out_f, lam)
        finally:
            _C.set_sh_cache(was)
        tag = f" [P={P} M={M} lam={lam} cache={cache}]"
        for t in ge:
            assert not torch.isnan(t).any(), "dense entry left an element unwritten" + tag
        for k in gn:
            assert not torch.isnan(gn[k]).any(), k + tag
        dsh = ge[5]
        assert dsh.shape == (P, M, 3)
        gp.grads_close("dL_dsh" + tag, r32["dL_dsh"].reshape(P, M, 3), dsh, gp.GRAD_REL, per_element=True)
        gp.grads_close("dL_dsh [hip vs f64]" + tag, r64["dL_dsh"].reshape(P, M, 3), dsh.double(), gp.GRAD_REL, per_element=True)
        gp.grads_close("dL_dmeans3D" + tag, r32["dL_dmeans3D"], ge[3], gp.GRAD_REL, per_element=True)   # the view-direction term
        assert (dsh[~vis] == 0).all() and (dsh[above] == 0).all() and dsh.abs().max() > 0
        # the split entry, bit for bit: both of its routes to the caller
        for dc, rest in ((gf[3], gf[4]), (gn["dc"], gn["rest"])):
            assert pg.bits_equal(dc, dsh[:, :1].contiguous()), "dL_dfeatures_dc" + tag
            assert rest.shape == (P, M - 1, 3)
            if M > 1:
                assert pg.bits_equal(rest, dsh[:, 1:].contiguous()), "dL_dfeatures_rest" + tag
        assert pg.bits_equal(gf[2], ge[3]) and pg.bits_equal(gn["m3d"], ge[3]), "dL_dmeans3D" + tag


def test_ragged_forward_spans_that_start_on_and_off_a_multiple_of_four():
    """The ragged (degree-sorted) SH store: per-degree counts chosen so that the spans of the waves after the first start at
    float offsets 192, 906, 2604 and 5634 -- two multiples of four and two that are not -- with lengths of both kinds.  Equal
    to the dense forward of the same Gaussians, as test_ragged_inference_path_reserved_equals_exact_equals_dense demands."""
    from diff_gaussian_rasterization import _C
    counts = (70, 60, 64, 65)
    P = sum(counts)
    cam, g = host_scene(P, 16)
    g = {k: g[k] for k in ("means3D", "sh", "opacity", "scales", "rotations")}
    g["degrees"] = np.repeat(np.arange(4, dtype=np.int32), counts).reshape(P, 1)
    g, flat, per_band, cumsum, coeffs = gp.ragged_inputs(g)
    assert tuple(per_band) == counts
    row_floats = 3 * (g["degrees"].reshape(-1).astype(np.int64) + 1) ** 2
    first = np.concatenate([[0], np.cumsum(row_floats)])[:P:64]          # float offset of each wave's span
    length = np.add.reduceat(row_floats, np.arange(0, P, 64))
    assert {int(f) % 4 == 0 for f in first[1:]} == {True, False} and {int(n) % 4 == 0 for n in length} == {True, False}
    bg = np.array([0.2, 0.3, 0.4], np.float32)
    _, dense = gp.hip_forward(_C, bg, g, cam, H, W, exact=True)
    assert (dense[2] > 0).any() and (dense[2] == 0).any()
    for w0 in range(0, P, 64):
        assert (dense[2][w0:w0 + 64] > 0).any(), "every wave has to stage its span"
    exd = _C.export_binning(P, dense[0], H, W, dense[3], dense[4], dense[5])
    for exact in (True, False, False):
        o = gp.hip_forward_ragged(_C, bg, g, flat, per_band, cumsum, coeffs, cam, H, W, exact=exact)
        assert int(o[0]) == int(dense[0]) and o[0].pairs == dense[0].pairs
        assert torch.equal(o[1], dense[1]) and torch.equal(o[2], dense[2])
        ex = _C.export_binning(P, o[0], H, W, o[3], o[4], o[5])
        for k in ("keys", "point_list", "ranges", "n_contrib", "final_T", "tiles_touched"):
            assert torch.equal(ex[k], exd[k]), k


@pytest.mark.parametrize("M", [4, 16])
def test_colour_variance_accumulate_step(M):
    """One camera = one accumulate step of colour_variance_accumulate_kernel, at two full waves and a wave of two rows."""
    P = 130
    cam, g = host_scene(P, M)
    a = dict(cam_positions=cam.camera_center[None], means3D=g["means3D"], opacity=g["opacity"], scales=g["scales"],
             rotations=g["rotations"], cam_viewmatrices=cam.world_view_transform[None], cam_projmatrices=cam.full_proj_transform[None],
             tan_fovxs=np.array([cam.tanfovx], np.float32), tan_fovys=np.array([cam.tanfovy], np.float32),
             image_height=np.array([H], np.int32), image_width=np.array([W], np.int32), sh=g["sh"], degrees=g["degrees"],
             max_sh_deg=math.isqrt(M) - 1)
    check_gpu_against_oracle(a)
