"""GPU checks of the fused L1 + D-SSIM loss (reduced-3dgs_amd/r3dgs_loss.py, csrc/loss.hip): the reference's recorded values,
float64 parity over shapes (tile edges, smaller than the window, one pixel) and value ranges, determinism, the two bindings,
graph capture, and a rasterizer training step against the reference's torch formula."""
import os

import numpy as np
import pytest
import torch

import r3dgs_loss
from diff_gaussian_rasterization import _C
from tests import loss_ref

pytestmark = pytest.mark.gpu

LAM = 0.2
SHAPES = [(3, 1062, 1600), (3, 1080, 1920), (2, 3, 37, 131), (1, 3, 5, 7), (1, 1, 1, 1), (1, 3, 16, 64), (1, 3, 17, 65)]
VALUE_SETS = ["unrelated", "near", "bright"]


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_grad(got, ref64, ref32, what):
    """Against float64, allowing for what the reference's own fp32 arithmetic (ref32, same inputs) gets wrong:
      max error <= max(1e-4 max|ref|, 2 x the fp32 reference's max error);
      per element |err| <= 1e-4 |ref| + max(1e-6 max|ref|, 2 x the fp32 reference's 99.9th-percentile error)
      on >= 99.9 % of the elements.
    The gradient of the SSIM *map* under a random per-pixel upstream, for near-identical pairs, is a sum of nearly cancelling
    terms: the reference's fp32 arithmetic meets `1e-4 |ref| + 1e-6 max|ref|` on only 59-97 % of its elements there
    (1e-6 dominates everywhere else, e.g. for every l1_dssim gradient)."""
    m = np.abs(ref64).max()
    err = np.abs(got - ref64)
    err32 = np.abs(ref32 - ref64)
    bar = max(1e-4 * m, 2.0 * err32.max())
    assert err.max() <= bar, f"{what}: max error {err.max():.3e} > {bar:.3e} (max|ref| {m:.3e})"
    slack = max(1e-6 * m, 2.0 * float(np.quantile(err32, 0.999)))
    frac = float(np.mean(err <= 1e-4 * np.abs(ref64) + slack))
    frac32 = float(np.mean(err32 <= 1e-4 * np.abs(ref64) + slack))
    assert frac >= 0.999, f"{what}: only {frac:.5f} of the elements within the per-element bar (fp32 reference: {frac32:.5f})"


def test_reference_fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, "ref_loss_grad.npz"))
    x = dv(d["image"]).requires_grad_()
    loss, l1, lssim = r3dgs_loss.l1_dssim(x, dv(d["gt"]), LAM)
    loss.backward()
    assert abs(l1.item() - float(d["l1"])) <= 1e-6
    assert abs((1.0 - lssim.item()) - float(d["ssim"])) <= 1e-6
    assert abs(loss.item() - float(d["loss"])) <= 1e-6
    g = d["dloss_dimage"]
    assert np.abs(x.grad.cpu().numpy() - g).max() <= 1e-5 * np.abs(g).max()
    s = r3dgs_loss.ssim(dv(d["image"]), dv(d["gt"]))
    assert abs(s.item() - float(d["ssim"])) <= 1e-6
    assert abs(r3dgs_loss.l1_loss(dv(d["image"]), dv(d["gt"])).item() - float(d["l1"])) <= 1e-6


@pytest.mark.parametrize("values", VALUE_SETS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_float64_parity(shape, values):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    x, y = loss_ref.value_set(values, shape, seed=sum(shape))
    rng = np.random.default_rng(11)
    up_map = rng.normal(0, 1, shape).astype(np.float32)
    B = shape[0] if len(shape) == 4 else 1
    up_img = rng.normal(0, 1, B).astype(np.float32)
    r64 = loss_ref.evaluate(x, y, torch.float64, LAM, upstream=up_map, per_image_upstream=up_img if len(shape) == 4 else None)
    r32 = loss_ref.evaluate(x, y, torch.float32, LAM, upstream=up_map, per_image_upstream=up_img if len(shape) == 4 else None)

    xt = dv(x).requires_grad_()
    loss, l1, lssim = r3dgs_loss.l1_dssim(xt, dv(y), LAM)
    loss.backward()
    assert abs(l1.item() - r64["l1"]) <= 1e-6
    assert abs((1.0 - lssim.item()) - r64["ssim"]) <= 1e-6
    assert abs(loss.item() - r64["loss"]) <= 1e-6
    check_grad(xt.grad.cpu().numpy(), r64["dloss"], r32["dloss"], "l1_dssim")

    xt = dv(x).requires_grad_()
    m = r3dgs_loss.ssim(xt, dv(y), aggregate=False)
    assert m.shape == xt.shape
    assert np.abs(m.detach().cpu().numpy() - r64["map"]).max() <= 1e-4
    m.backward(dv(up_map))
    check_grad(xt.grad.cpu().numpy(), r64["dmap"], r32["dmap"], "ssim map")

    if len(shape) == 4:
        xt = dv(x).requires_grad_()
        s = r3dgs_loss.ssim(xt, dv(y), size_average=False)
        assert s.shape == (B,)
        assert np.abs(s.detach().cpu().numpy() - r64["ssim_image"]).max() <= 1e-6
        s.backward(dv(up_img))
        check_grad(xt.grad.cpu().numpy(), r64["dimage"], r32["dimage"], "ssim per image")


@pytest.mark.parametrize("shape", [(3, 64, 80), (2, 3, 37, 131)], ids=["3x64x80", "2x3x37x131"])
def test_image_equal_to_its_target(shape):
    x = loss_ref.value_set("unrelated", shape, seed=5)[0]
    n = x.size
    xt = dv(x).requires_grad_()
    loss, l1, lssim = r3dgs_loss.l1_dssim(xt, dv(x), LAM)
    loss.backward()
    assert l1.item() == 0.0
    assert abs(lssim.item()) <= 1e-6     # mean SSIM 1
    assert xt.grad.abs().max().item() <= 1e-4 * (1 - LAM) / n
    xt = dv(x).requires_grad_()
    r3dgs_loss.l1_loss(xt, dv(x)).backward()
    assert torch.count_nonzero(xt.grad).item() == 0   # sign(0) = 0: the L1 gradient is exactly 0


def _all_forms(x, y, up_map):
    out = []
    xt = x.clone().requires_grad_()
    loss, l1, lssim = r3dgs_loss.l1_dssim(xt, y, LAM)
    loss.backward()
    out += [loss, l1, lssim, xt.grad]
    xt = x.clone().requires_grad_()
    m = r3dgs_loss.ssim(xt, y, aggregate=False)
    m.backward(up_map)
    out += [m.detach(), xt.grad]
    xt = x.clone().requires_grad_()
    s = r3dgs_loss.ssim(xt, y, size_average=False)
    s.sum().backward()
    out += [s.detach(), xt.grad]
    xt = x.clone().requires_grad_()
    s = r3dgs_loss.l1_loss(xt, y)
    s.backward()
    out += [s.detach(), xt.grad]
    torch.cuda.synchronize()
    return [t.detach().clone() for t in out]


def test_deterministic_and_both_bindings_identical():
    x, y = (dv(a) for a in loss_ref.value_set("near", (2, 3, 300, 421), seed=2))
    up = dv(np.random.default_rng(1).normal(0, 1, (2, 3, 300, 421)).astype(np.float32))
    first = _all_forms(x, y, up)
    second = _all_forms(x, y, up)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert _C.binding() == "torch"
    was = _C.set_binding("ctypes")
    try:
        via_ctypes = _all_forms(x, y, up)
    finally:
        _C.set_binding(was)
    for a, b in zip(first, via_ctypes):
        assert torch.equal(a, b)


def test_graph_capture_equals_eager():
    shape = (3, 240, 320)
    x0, y0 = loss_ref.value_set("unrelated", shape, seed=7)
    x1, y1 = loss_ref.value_set("near", shape, seed=8)
    xs = dv(x0).requires_grad_()
    ys = dv(y0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = None
            r3dgs_loss.l1_dssim(xs, ys, LAM)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, l1, lssim = r3dgs_loss.l1_dssim(xs, ys, LAM)
        loss.backward()
    with torch.no_grad():
        xs.copy_(dv(x1))
        ys.copy_(dv(y1))
    g.replay()
    torch.cuda.synchronize()
    xe = dv(x1).requires_grad_()
    le, l1e, lse = r3dgs_loss.l1_dssim(xe, dv(y1), LAM)
    le.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss, le) and torch.equal(l1, l1e) and torch.equal(lssim, lse)
    assert torch.equal(xs.grad, xe.grad)


def test_training_step_end_to_end():
    """Rasterizer forward -> fused l1_dssim -> backward against rasterizer forward -> the reference's torch formula ->
    backward, on one synth_scene workload: every parameter gradient within 1e-4 max|ref|."""
    import diff_gaussian_rasterization as dgr
    import synth_scene as ss
    w, cam, g = ss.make_workload("cfg0_10k_400", seed=0)
    W, H = w["W"], w["H"]
    degrees = dv(g["degrees"])
    empty = torch.Tensor([])
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dv(np.zeros(3, np.float32)), 1.0,
                                           dv(cam.world_view_transform), dv(cam.full_proj_transform), 3,
                                           dv(cam.camera_center), False, False)
    gt = dv(np.random.default_rng(3).random((3, H, W)).astype(np.float32))

    def step(loss_fn):
        leaves = {k: dv(g[k]).requires_grad_() for k in ("means3D", "opacity", "scales", "rotations", "sh")}
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
        means2D.retain_grad()
        color, _ = dgr.rasterize_gaussians(leaves["means3D"], means2D, leaves["sh"], degrees, empty, leaves["opacity"],
                                           leaves["scales"], leaves["rotations"], empty, rs, 0.0)
        loss = loss_fn(color, gt)[0]
        loss.backward()
        grads = {k: v.grad.cpu().numpy() for k, v in leaves.items()}
        grads["means2D"] = means2D.grad.cpu().numpy()
        return loss.item(), grads

    loss_f, fused = step(lambda c, t: r3dgs_loss.l1_dssim(c, t, LAM))
    loss_t, torch_f = step(lambda c, t: loss_ref.torch_formula(c, t, LAM))
    assert abs(loss_f - loss_t) <= 1e-6
    for k, ref in torch_f.items():
        m = np.abs(ref).max()
        assert m > 0, k
        assert np.abs(fused[k] - ref).max() <= 1e-4 * m, k
