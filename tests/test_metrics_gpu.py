"""GPU tests (-m gpu) of the evaluation metrics (reduced-3dgs_amd/r3dgs_metrics.py, csrc/metrics.hip): float64 parity of
image_metrics over the shapes at which a tiled window kernel and a strided reduction go wrong, every ground-truth layout and
flag combination, infinities and NaN, the drop-in psnr / mse and to_uint8 against the reference's recorded output, determinism,
graph capture, and evaluate() over a camera set for a dense and a quantised model.

The kernel's tile is 64 x 16 (csrc/ssim_tile.h kTW, kTH), so the shapes are the issue's: one pixel; 3x17x70, one pixel past a
tile edge in each direction; 3x5x3, smaller than the window; the fixture's 3x40x56; 4x33x130; and 2x64x64, exact tiles.

Bars, all against tests/metrics_ref.py fed the same arrays (n = the element count of the mean in question):
  l1, mse, mse_c   n 2^-52 relative: the worst case of reordering a sum of n non-negative doubles whose terms are computed
                   identically on both sides
  ssim             1e-6 absolute (tests/test_loss_gpu.py)
  psnr_*           10 log10(e) (n 2^-52 + 2^-52) dB when finite; equal when infinite; NaN where the restatement is NaN"""
import ctypes
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import r3dgs_metrics as rm
from diff_gaussian_rasterization import _C
from tests import metrics_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 17, 70), (3, 5, 3), (3, 40, 56), (4, 33, 130), (2, 64, 64)]
PARITY_SHAPES = SHAPES + [(3, 16, 64), (3, 17, 65)]   # exactly one tile; one pixel past the tile edge in both directions
LAYOUTS = {"f32": _C.GT_F32_CHW, "u8_chw": _C.GT_U8_CHW, "u8_hwc": _C.GT_U8_HWC}
DB = 10.0 * math.log10(math.e)
U = 2.0 ** -52
EPS32 = 2.0 ** -24


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def inputs(shape, seed):
    """image in [-0.2, 1.3]; a float truth in [-0.1, 1.1] (so that clamping it matters) and random bytes in both layouts"""
    rng = np.random.default_rng(seed)
    image = rng.uniform(-0.2, 1.3, shape).astype(np.float32)
    gts = {"f32": rng.uniform(-0.1, 1.1, shape).astype(np.float32)}
    gts["u8_chw"] = rng.integers(0, 256, shape, dtype=np.uint8)
    gts["u8_hwc"] = np.ascontiguousarray(gts["u8_chw"].transpose(1, 2, 0))
    return image, gts


def run(image_t, gt_t, layout, clamp, quantise):
    """image_metrics through the Python surface; a uint8 truth whose shape reads as both layouts (C == H == W: refused there
    unless it is one sample) through the binding with the layout spelled out."""
    C, H, W = image_t.shape
    if layout != "f32" and C == H == W:
        out = torch.empty(rm.ROW, dtype=torch.float64, device="cuda")
        ws = torch.empty(_C.image_metrics_workspace_bytes(C, H, W), dtype=torch.uint8, device="cuda")
        return _C.image_metrics(image_t, gt_t, LAYOUTS[layout], (1 if clamp else 0) | (2 if quantise else 0), out, ws)
    return rm.image_metrics(image_t, gt_t, clamp=clamp, quantise=quantise)


def check_row(got, ref, shape, what):
    """got: float64 [ROW] numpy; ref: metrics_ref.row's dict."""
    C, H, W = shape
    n_all, n_plane = C * H * W, H * W
    for k, name in enumerate(rm.FIELDS):
        g, r = float(got[k]), ref[name]
        print(f"{what} {name}: got {g!r} ref {r!r}")
        if math.isnan(r):
            assert math.isnan(g), (what, name, g)
            continue
        if math.isinf(r):
            assert g == r, (what, name, g)
            continue
        n = n_all if name in ("l1", "mse", "psnr_image", "ssim") else n_plane
        if name == "ssim":
            assert abs(g - r) <= 1e-6, (what, name, g, r)
        elif name.startswith("psnr"):
            assert abs(g - r) <= DB * (n * U + U), (what, name, g, r, abs(g - r))
        else:
            assert abs(g - r) <= n * U * abs(r), (what, name, g, r)


@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=["x".join(map(str, s)) for s in PARITY_SHAPES])
def test_image_metrics_float64_parity(shape):
    image, gts = inputs(shape, seed=sum(shape))
    xt = dv(image)
    for layout, gt in gts.items():
        gt_t = dv(gt)
        for clamp in (False, True):
            for quantise in (False, True):
                got = run(xt, gt_t, layout, clamp, quantise)
                assert got.dtype == torch.float64 and got.shape == (rm.ROW,) and got.is_cuda
                ref = metrics_ref.row(image, gt, layout, clamp, quantise)
                check_row(got.cpu().numpy(), ref, shape, (shape, layout, clamp, quantise))
                assert all(float(got[2 + c]) == 0.0 for c in range(shape[0], 4))
                again = run(xt, gt_t, layout, clamp, quantise)   # determinism: identical bits
                assert torch.equal(got.view(torch.int64), again.view(torch.int64))


def test_out_row_is_written_in_place_and_layout_is_detected():
    shape = (3, 17, 70)
    image, gts = inputs(shape, seed=3)
    xt = dv(image)
    table = torch.zeros(2, rm.ROW, dtype=torch.float64, device="cuda")
    ret = rm.image_metrics(xt, dv(gts["u8_hwc"]), out=table[1])
    assert ret.data_ptr() == table[1].data_ptr() and not table[0].any()
    assert torch.equal(table[1], rm.image_metrics(xt, dv(gts["u8_chw"])))   # the same bytes, the other layout
    assert not torch.equal(table[1], rm.image_metrics(xt, dv(gts["f32"])))
    with pytest.raises(ValueError, match="not contiguous"):
        rm.image_metrics(xt[:, :, ::2], dv(gts["f32"])[:, :, ::2])
    with pytest.raises(ValueError, match="not contiguous"):
        rm.image_metrics(xt, dv(gts["u8_chw"]).permute(1, 2, 0))
    with pytest.raises(ValueError, match="out must be"):
        rm.image_metrics(xt, dv(gts["f32"]), out=torch.zeros(rm.ROW, device="cuda"))
    with pytest.raises(ValueError, match="ambiguous"):
        rm.image_metrics(torch.rand(3, 3, 3, device="cuda"), torch.zeros(3, 3, 3, dtype=torch.uint8, device="cuda"))


def test_identical_images_give_infinite_psnr():
    shape = (3, 17, 70)
    _, gts = inputs(shape, seed=4)
    y = metrics_ref.from_u8(gts["u8_chw"])          # floats that are exactly byte / 255
    for gt_t in (dv(y), dv(gts["u8_chw"]), dv(gts["u8_hwc"])):
        for quantise in (False, True):
            row = rm.image_metrics(dv(y), gt_t, quantise=quantise).cpu().numpy()
            named = dict(zip(rm.FIELDS, row))
            assert named["psnr_image"] == math.inf and named["psnr_channels"] == math.inf
            assert named["l1"] == 0.0 and named["mse"] == 0.0 and abs(named["ssim"] - 1.0) <= 1e-6


def test_nan_propagates():
    shape = (3, 17, 70)
    image, gts = inputs(shape, seed=5)
    image[1, 5, 7] = np.nan
    for layout in ("f32", "u8_hwc"):
        for clamp in (False, True):
            got = run(dv(image), dv(gts[layout]), layout, clamp, False).cpu().numpy()
            ref = metrics_ref.row(image, gts[layout], layout, clamp, False)
            for name in ("l1", "mse", "mse_c1", "psnr_image", "psnr_channels", "ssim"):
                assert math.isnan(ref[name])
            assert not math.isnan(ref["mse_c0"]) and not math.isnan(ref["mse_c2"])
            check_row(got, ref, shape, ("nan", layout, clamp))
        # the 8-bit rounding maps NaN to 0 (include/r3dgs_metrics.h): nothing is NaN
        got = run(dv(image), dv(gts[layout]), layout, True, True).cpu().numpy()
        assert not np.isnan(got).any()
        check_row(got, metrics_ref.row(image, gts[layout], layout, True, True), shape, ("nan quantised", layout))
    gt = gts["f32"].copy()
    gt[2, 16, 69] = np.nan                           # the last element of a float truth
    got = run(dv(inputs(shape, 5)[0]), dv(gt), "f32", True, False).cpu().numpy()
    check_row(got, metrics_ref.row(inputs(shape, 5)[0], gt, "f32", True, False), shape, "nan in gt")
    assert math.isnan(got[rm.FIELDS.index("mse_c2")]) and not math.isnan(got[rm.FIELDS.index("mse_c0")])


def _psnr_fixture_bar(p):
    """tests/test_metrics_cpu.py: the reference's fp32 mse is within 8 x 2^-24 relative, and two ulps of the recorded value"""
    p = np.float32(abs(p))
    return DB * 8 * EPS32 + 2 * float(np.nextafter(p, np.float32(np.inf)) - p)


def _half_ulp32(v):
    v = np.float32(abs(v))
    return 0.5 * float(np.nextafter(v, np.float32(np.inf)) - v)


def test_psnr_and_mse_drop_ins(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_metrics.npz"))
    image, gt = d["image"], d["gt"]
    ci, cg = metrics_ref.clamp01(image), metrics_ref.clamp01(gt)
    rng = np.random.default_rng(9)
    cases = [(ci, cg, "chw"), (ci[None], cg[None], "bchw"), (image, gt, "raw_chw"),
             (rng.random((5, 7), dtype=np.float32), rng.random((5, 7), dtype=np.float32), None),
             # rows longer than one chunk of the kernel (4096 elements) and not a multiple of it; a single long row
             (rng.random((3, 9000), dtype=np.float32), rng.random((3, 9000), dtype=np.float32), None),
             (rng.random((1, 2, 4097), dtype=np.float32), rng.random((1, 2, 4097), dtype=np.float32), None),
             (rng.random((6,), dtype=np.float32), rng.random((6,), dtype=np.float32), None)]
    for a, b, key in cases:
        m, p = rm.mse(dv(a), dv(b)), rm.psnr(dv(a), dv(b))
        rows = a.shape[0]
        n = a.size // rows
        for t in (m, p):
            assert t.shape == (rows, 1) and t.dtype == torch.float32 and t.is_cuda
        m, p = m.cpu().numpy().astype(np.float64)[:, 0], p.cpu().numpy().astype(np.float64)[:, 0]
        m64, p64 = metrics_ref.row_mse(a, b), metrics_ref.row_psnr(a, b)
        for i in range(rows):
            print(f"{key} {a.shape} row {i}: mse {m[i]!r} ref {m64[i]!r}; psnr {p[i]!r} ref {p64[i]!r}")
            # the double row mean (n 2^-52 relative) rounded once to fp32
            assert abs(m[i] - m64[i]) <= n * U * m64[i] + _half_ulp32(m64[i])
            # ... and the four double operations of the formula, each within an ulp of a value no larger than 2 |psnr|
            assert abs(p[i] - p64[i]) <= DB * n * U + 8 * U * abs(p64[i]) + _half_ulp32(p64[i])
            if key is not None:
                rm_ref, rp_ref = float(d["mse_" + key][i, 0]), float(d["psnr_" + key][i, 0])
                assert abs(m[i] - rm_ref) <= 8 * EPS32 * m64[i] + _half_ulp32(m64[i])
                assert abs(p[i] - rp_ref) <= _psnr_fixture_bar(rp_ref) + _half_ulp32(rp_ref)
        assert torch.equal(rm.mse(dv(a), dv(b)), rm.mse(dv(a), dv(b)))
    # the two PSNR conventions of the fused row are the drop-ins on the two forms of the clamped pair
    row = dict(zip(rm.FIELDS, rm.image_metrics(dv(image), dv(gt)).cpu().numpy()))
    assert abs(row["psnr_image"] - float(d["psnr_bchw"][0, 0])) <= _psnr_fixture_bar(d["psnr_bchw"][0, 0])
    assert abs(row["psnr_channels"] - float(d["psnr_chw"].astype(np.float64).mean())) <= \
        max(_psnr_fixture_bar(v) for v in d["psnr_chw"][:, 0])
    assert abs(row["l1"] - float(d["l1"])) <= 8 * EPS32 * row["l1"]
    assert abs(row["ssim"] - float(d["ssim"])) <= 1e-6
    with pytest.raises(ValueError, match="not contiguous"):
        rm.psnr(dv(ci)[:, ::2], dv(cg)[:, ::2])


def test_to_uint8(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_metrics.npz"))
    got = rm.to_uint8(dv(d["image"]))
    assert got.shape == (40, 56, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), d["bytes_chw"].transpose(1, 2, 0))
    for shape in SHAPES:
        image, _ = inputs(shape, seed=7 + sum(shape))
        image.reshape(-1)[::5] = (np.arange(image.size)[::5] % 256 + 0.5).astype(np.float32) / np.float32(255.0)   # ties
        xt = dv(image)
        want = xt.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0)
        got = rm.to_uint8(xt)
        assert got.shape == (shape[1], shape[2], shape[0]) and torch.equal(got, want), shape
        assert np.array_equal(got.cpu().numpy(), metrics_ref.quantise8(image).transpose(1, 2, 0))


def _hip():
    """The HIP runtime this process already runs on."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    assert path, "no HIP runtime loaded"
    return ctypes.CDLL(path)


def test_graph_capture_replays_on_new_contents_and_is_one_chain():
    shape = (3, 40, 56)
    image0, gts = inputs(shape, seed=21)
    image1, _ = inputs(shape, seed=22)
    xs, gt_t = dv(image0), dv(gts["u8_hwc"])
    out = torch.zeros(rm.ROW, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            rm.image_metrics(xs, gt_t, quantise=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        rm.image_metrics(xs, gt_t, quantise=True, out=out)
    # the capture: the tile kernel and the finishing launch, one after the other -- no parallel branches
    hip = _hip()
    graph = ctypes.c_void_p(g.raw_cuda_graph())
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(n_edges)) == 0
    assert n_nodes.value == 2 and n_edges.value == 1, (n_nodes.value, n_edges.value)
    roots = ctypes.c_size_t(0)
    assert hip.hipGraphGetRootNodes(graph, None, ctypes.byref(roots)) == 0 and roots.value == 1
    xs.copy_(dv(image1))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    fresh = rm.image_metrics(dv(image1), gt_t, quantise=True)
    assert torch.equal(out.view(torch.int64), fresh.view(torch.int64))
    assert not torch.equal(out, rm.image_metrics(dv(image0), gt_t, quantise=True))


# ---- evaluate(): V = 3 cameras at 64 x 48 over the 200-Gaussian fixture model, dense (its decoded tensors) and quantised

VIEWS = [(0.1, -0.05, 4.0), (-0.2, 0.1, 4.5), (0.0, 0.05, 3.5)]
PIPE = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _cameras(gt_of):
    import synth_scene as ss
    cams = []
    for v, T in enumerate(VIEWS):
        cam = ss.Camera(64, 48, 60.0, 60.0, None, T)
        cams.append(NS(image_height=48, image_width=64, FoVx=cam.FoVx, FoVy=cam.FoVy,
                       world_view_transform=dv(cam.world_view_transform), full_proj_transform=dv(cam.full_proj_transform),
                       camera_center=dv(cam.camera_center), original_image=gt_of(v)))
    return cams


@pytest.fixture(scope="module")
def models(golden_dir):
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    dense = NS(**qm.decode(), active_sh_degree=3, max_sh_degree=3)
    return {"dense": dense, "quantised": qm}


@pytest.mark.parametrize("kind", ["dense", "quantised"])
def test_evaluate(models, kind):
    import r3dgs_render
    model = models[kind]
    assert model._xyz.shape[0] == 200 if kind == "dense" else model.P == 200
    bg = dv(np.array([0.1, 0.2, 0.3], np.float32))
    rng = np.random.default_rng(31)
    gt_u8 = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in VIEWS]                  # [H,W,C] bytes
    gt_f32 = [metrics_ref.from_u8(np.ascontiguousarray(g.transpose(2, 0, 1))) for g in gt_u8]   # the same, pre-divided
    cams_u8 = _cameras(lambda v: dv(gt_u8[v]))
    cams_f32 = _cameras(lambda v: dv(gt_f32[v]))
    res = rm.evaluate(cams_f32, model, PIPE, bg)
    table = res["per_view"]
    assert set(res) == {"per_view", "mean", "fields"} and res["fields"] == rm.FIELDS
    assert table.shape == (3, rm.ROW) and table.dtype == torch.float64 and table.is_cuda
    assert torch.equal(res["mean"], table.mean(0))
    renders = []
    for v, cam in enumerate(cams_f32):
        with torch.no_grad():
            image = r3dgs_render.render(cam, model, PIPE, bg)["render"]
        renders.append(image)
        assert image.shape == (3, 48, 64) and (image != bg[:, None, None]).any(), "the view must show the model"
        # row v is image_metrics of render(camera_v), bit for bit
        assert torch.equal(table[v].view(torch.int64), rm.image_metrics(image, cam.original_image).view(torch.int64))
        check_row(table[v].cpu().numpy(), metrics_ref.row(image.cpu().numpy(), gt_f32[v], "f32", True, False), (3, 48, 64),
                  (kind, "view", v))
    assert not torch.equal(table[0], table[1])
    # the truth stored as the decoder's bytes gives the same table as the same bytes pre-divided to float
    res_u8 = rm.evaluate(cams_u8, model, PIPE, bg)
    assert torch.equal(res_u8["per_view"].view(torch.int64), table.view(torch.int64)), "uint8 truth != pre-divided float truth"
    # quantise=True: the render rounded by to_uint8 and read back through the uint8 load
    res_q = rm.evaluate(cams_u8, model, PIPE, bg, quantise=True)
    for v, image in enumerate(renders):
        # byte / 255 on the host: torch's device division by a Python scalar multiplies by the rounded reciprocal, which is
        # not to_tensor's correctly rounded divide
        back = dv(metrics_ref.from_u8(np.ascontiguousarray(rm.to_uint8(image).cpu().numpy().transpose(2, 0, 1))))
        want = rm.image_metrics(back, cams_u8[v].original_image, clamp=True, quantise=False)
        assert torch.equal(res_q["per_view"][v].view(torch.int64), want.view(torch.int64)), \
            ("quantise=True != to_uint8 bytes read back", v, res_q["per_view"][v].tolist(), want.tolist())
        check_row(res_q["per_view"][v].cpu().numpy(), metrics_ref.row(image.cpu().numpy(), gt_u8[v], "u8_hwc", True, True),
                  (3, 48, 64), (kind, "quantised view", v))
    assert not torch.equal(res_q["per_view"], table)
    # a render function of the caller's is used in place of r3dgs_render.render
    calls = []

    def my_render(camera, pc, pipe, background):
        calls.append(camera)
        return {"render": renders[len(calls) - 1]}
    res_r = rm.evaluate(cams_f32, model, PIPE, bg, render=my_render)
    assert len(calls) == 3 and torch.equal(res_r["per_view"].view(torch.int64), table.view(torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rm.evaluate(_cameras(lambda v: torch.from_numpy(gt_f32[v])), model, PIPE, bg)
