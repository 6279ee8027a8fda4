"""GPU checks of the exposure + mask loss (reduced-3dgs_amd/r3dgs_exposure.py, the exposure kernels of csrc/loss.hip) against the
float64 restatement tests/exposure_loss_ref.py, at the project's standing bars:
    values      loss, Ll1, Lssim within 1e-5 absolute
    gradients   d image and d exposure each within 1e-4 * max|ref| of the float64 autograd gradient, no element excluded
    exactness   without exposure and mask, and with E = eye(3,4) and a mask of ones, the bits of r3dgs_loss.l1_dssim; both
                bindings, two runs, a 0xFF-filled workspace and a replayed torch.cuda.graph give the same bits, dE included
Shapes: the smallest that reach every edge of the 64 x 16 tile with its 5-pixel halo -- 3x40x70 (2 x 3 tiles, ragged both ways),
3x130x23 (portrait, one ragged column), 3x16x64 (exactly one tile), 3x1x1, and a batch of two 3x40x70 images with per-image and
with shared exposure and mask.  Inputs: exposure_loss_ref.inputs (a smooth target, the prediction under a deliberately wrong
exposure plus noise, a mask with ~30 % zeros); tests/test_exposure_loss_cpu.py holds the recipe's smallest dE entry to 5 % of the
largest.  Measured worst figures: profiles/exposure_loss_gpu_tests.txt."""
import numpy as np
import pytest
import torch

from tests import exposure_loss_ref as ref

pytestmark = pytest.mark.gpu
LAM = 0.2
SINGLE = [(3, 40, 70), (3, 130, 23), (3, 16, 64), (3, 1, 1)]


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _run(x, y, E=None, m=None, mask_target=False, lam=LAM):
    """One fused forward + backward on device tensors -> [loss, l1, lssim, dx, dE or None], detached clones."""
    import r3dgs_exposure
    xt = x.detach().clone().requires_grad_()
    Et = None if E is None else E.detach().clone().requires_grad_()
    loss, l1, lssim = r3dgs_exposure.exposed_l1_dssim(xt, y, Et, m, mask_target, lam)
    assert not l1.requires_grad and not lssim.requires_grad and loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    return [loss.detach().clone(), l1.clone(), lssim.clone(), xt.grad.clone(), None if Et is None else Et.grad.clone()]


def _hold(got, want, what):
    """The bars of the module docstring; prints the figures before it asserts."""
    loss, l1, lssim, dx, dE = got
    ev = max(abs(loss.item() - want["loss"]), abs(l1.item() - want["l1"]), abs(lssim.item() - want["lssim"]))
    top_x = np.abs(want["dx"]).max()
    ex = np.abs(dx.cpu().numpy().astype(np.float64) - want["dx"]).max() / top_x
    line = f"exposure loss {what}: values {ev:.2e} (bar 1e-5), d image {ex:.2e} of max|ref| (bar 1e-4)"
    ee = None
    if want["dE"] is not None:
        top_e = np.abs(want["dE"]).max()
        ee = np.abs(dE.cpu().numpy().astype(np.float64) - want["dE"]).max() / top_e
        line += f", d exposure {ee:.2e} of max|ref| (bar 1e-4)"
        assert top_e > 0
    print(line)
    assert top_x > 0 and ev <= 1e-5 and ex <= 1e-4, line
    assert ee is None or ee <= 1e-4, line


@pytest.mark.parametrize("mask_target", [False, True], ids=["mask_prediction", "mask_both"])
@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(map(str, s)))
def test_float64_parity(shape, mask_target):
    x, y, m = ref.inputs(shape, seed=20 + shape[1])
    E = ref.exposure_guess(1, seed=3)[0]
    want = ref.evaluate(x, y, E, m, mask_target, LAM)
    _hold(_run(dv(x), dv(y), dv(E), dv(m[0]), mask_target), want, f"{shape} mask_target={mask_target}")


@pytest.mark.parametrize("which", ["exposure_only", "mask_only", "mask_only_one_channel"])
def test_float64_parity_one_input_absent(which):
    shape = (3, 40, 70)
    x, y, m = ref.inputs(shape, seed=31)
    E = ref.exposure_guess(1, seed=4)[0] if which == "exposure_only" else None
    m = None if which == "exposure_only" else m
    if which == "mask_only_one_channel":   # any C without an exposure
        x, y = x[:1], y[:1]
    want = ref.evaluate(x, y, E, m, True, LAM)
    _hold(_run(dv(x), dv(y), None if E is None else dv(E), None if m is None else dv(m[0, 0]), True), want, which)


@pytest.mark.parametrize("per_image", [True, False], ids=["per_image", "shared"])
def test_float64_parity_batch(per_image):
    shape = (2, 3, 40, 70)
    x, y, m = ref.inputs(shape, seed=41)
    E = ref.exposure_guess(2, seed=5)
    if not per_image:
        E, m = E[0], m[0]                      # [3,4] and [1,H,W]: one exposure, one mask for both images
    want = ref.evaluate(x, y, E, m, False, LAM)
    got = _run(dv(x), dv(y), dv(E), dv(m), False)
    assert got[4].shape == E.shape
    _hold(got, want, f"batch of 2, {'per-image' if per_image else 'shared'} exposure and mask")


@pytest.mark.parametrize("shape", SINGLE + [(2, 3, 40, 70), (2, 40, 70)], ids=lambda s: "x".join(map(str, s)))
def test_identity_is_l1_dssim_bit_for_bit(shape):
    """exposure=None, mask=None -- and E = eye(3,4), mask = ones -- give r3dgs_loss.l1_dssim's three values and gradient bit
    for bit; and r3dgs_loss.l1_dssim itself still gives what the untouched r3dgs_l1_ssim_* entry points give."""
    import r3dgs_loss
    from diff_gaussian_rasterization import _C
    if len(shape) == 4 or shape[0] == 3:
        x, y, _ = ref.inputs(shape, seed=50 + shape[-1])
    else:
        x, y, _ = ref.inputs((3,) + shape[1:], seed=50)
        x, y = x[:2], y[:2]
    x, y = dv(x), dv(y)
    xt = x.clone().requires_grad_()
    loss, l1, lssim = r3dgs_loss.l1_dssim(xt, y, LAM)
    loss.backward()
    plain = [loss.detach(), l1, lssim, xt.grad]
    # the existing surface: the same numbers through the C entry points r3dgs_loss has always called
    B, C, H, W = (1,) + tuple(shape) if len(shape) == 3 else shape
    l1_c, _, loss_c, dssim_c, _, _, partials = _C.l1_ssim_forward(x, y, B, C, H, W, LAM, True, False)
    one = torch.ones((), device="cuda")
    dx_c = _C.l1_ssim_backward(x, y, partials, one, 1.0 - LAM, one, 0, -LAM, B, C, H, W).view(x.shape)
    for a, b in zip(plain, [loss_c, l1_c, dssim_c, dx_c]):
        assert _bits_equal(a, b), "r3dgs_loss.l1_dssim no longer gives the bits of r3dgs_l1_ssim_*"
    bare = _run(x, y)
    for a, b in zip(plain, bare[:4]):
        assert _bits_equal(a, b), "exposure=None, mask=None differs from l1_dssim"
    ones = torch.ones(shape[-2:], device="cuda")
    for a, b in zip(plain, _run(x, y, None, ones, True)[:4]):
        assert _bits_equal(a, b), "a mask of ones differs from l1_dssim"
    if C == 3:
        eye = torch.eye(3, 4, device="cuda")
        for E in (eye, eye.expand(B, 3, 4).contiguous()):
            for a, b in zip(plain, _run(x, y, E, ones, False)[:4]):
                assert _bits_equal(a, b), "E = eye(3,4), mask = ones differs from l1_dssim"


def _batch_case():
    x, y, m = ref.inputs((2, 3, 40, 70), seed=61)
    return dv(x), dv(y), dv(ref.exposure_guess(2, seed=6)), dv(m)


def test_deterministic_and_both_bindings_identical():
    from diff_gaussian_rasterization import _C
    x, y, E, m = _batch_case()
    forms = lambda: _run(x, y, E, m, True) + _run(x, y, E[0], m[0], False) + _run(x, y, None, m, False)   # noqa: E731
    first, second = forms(), forms()
    assert _C.binding() == "torch"
    was = _C.set_binding("ctypes")
    try:
        via_ctypes = forms()
    finally:
        _C.set_binding(was)
    for a, b, c in zip(first, second, via_ctypes):
        assert (a is None and b is None and c is None) or (_bits_equal(a, b) and _bits_equal(a, c))


def test_workspace_contents_do_not_matter():
    """The C calls on a workspace filled with 0xFF and on one filled with zeros: the same bits, dE included."""
    from diff_gaussian_rasterization import _C
    x, y, E, m = _batch_case()
    B, C, H, W = x.shape
    g = torch.ones((), device="cuda")
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((_C.exposure_loss_workspace_bytes(B, C, H, W),), fill, dtype=torch.uint8, device="cuda")
        fwd = _C.exposure_loss_forward(x, y, E, True, m, True, False, B, C, H, W, LAM, True, _workspace=ws)
        ws.fill_(fill)
        bwd = _C.exposure_loss_backward(x, y, E, True, m, True, False, fwd[5], g, 1.0 - LAM, -LAM, True, B, C, H, W, _workspace=ws)
        torch.cuda.synchronize()
        outs.append(list(fwd) + list(bwd))
    for a, b in zip(*outs):
        assert _bits_equal(a, b)
    for a, b in zip(outs[0][:4] + outs[0][6:], (lambda r: [r[1], None, r[0], r[2], r[3], r[4]])(_run(x, y, E, m, False))):
        assert b is None or _bits_equal(a, b), "the C calls and the autograd surface disagree"


def test_graph_capture_equals_eager():
    """Forward + backward captured on a warmed side stream; the replay follows a changed image, target and exposure buffer."""
    import r3dgs_exposure
    x0, y0, m0 = ref.inputs((3, 40, 70), seed=71)
    x1, y1, _ = ref.inputs((3, 40, 70), seed=72)
    E0, E1 = ref.exposure_guess(2, seed=7)
    xs, ys, ms = dv(x0).requires_grad_(), dv(y0), dv(m0[0])
    Es = dv(E0).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            xs.grad = Es.grad = None
            r3dgs_exposure.exposed_l1_dssim(xs, ys, Es, ms, True, LAM)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = Es.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss, l1, lssim = r3dgs_exposure.exposed_l1_dssim(xs, ys, Es, ms, True, LAM)
        loss.backward()
    with torch.no_grad():
        xs.copy_(dv(x1))
        ys.copy_(dv(y1))
        Es.copy_(dv(E1))
    g.replay()
    torch.cuda.synchronize()
    eager = _run(dv(x1), dv(y1), dv(E1), ms, True)
    for a, b in zip([loss, l1, lssim, xs.grad, Es.grad], eager):
        assert _bits_equal(a, b)
    assert not _bits_equal(Es.grad, _run(dv(x1), dv(y1), dv(E0), ms, True)[4]), "the replay did not follow the exposure buffer"


@pytest.mark.parametrize("shape", [(3, 40, 70), (2, 3, 17, 65), (3, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_apply_exposure(shape):
    import r3dgs_exposure
    rng = np.random.default_rng(81)
    x = rng.uniform(-0.2, 1.2, shape).astype(np.float32)
    B = shape[0] if len(shape) == 4 else 1
    E = ref.exposure_guess(B, seed=8)
    E = E if len(shape) == 4 else E[0]
    want = ref.exposed(torch.from_numpy(x).double().reshape((-1,) + shape[-3:]), torch.from_numpy(E).double()).reshape(shape)
    got = r3dgs_exposure.apply_exposure(dv(x), dv(E))
    assert got.shape == shape and not got.requires_grad
    # 1e-6 of the sum of the magnitudes of a value's four terms (<= 1.2 * 3 * 1.3 + 0.3 here), the scale its rounding has
    scale = ref.exposed(torch.from_numpy(np.abs(x)).double().reshape((-1,) + shape[-3:]), torch.from_numpy(np.abs(E)).double()).reshape(shape)
    # and, since that scale passes 1 for the brightest pixels, plain 1e-6 absolute as well
    err = (got.cpu().double() - want).abs()
    print(f"apply_exposure {shape}: worst error {err.max().item():.2e} (bar 1e-6 absolute), {(err / scale).max().item():.2e} of the terms' magnitude")
    assert (err <= 1e-6 * scale).all() and err.max() <= 1e-6
    clamped = r3dgs_exposure.apply_exposure(dv(x), dv(E), clamp=True)
    err = (clamped.cpu().double() - want.clamp(0, 1)).abs()
    assert (err <= 1e-6 * scale).all() and err.max() <= 1e-6
    assert clamped.min() >= 0 and clamped.max() <= 1
    assert x.size < 100 or ((clamped == 0).any() and (clamped == 1).any()), "the inputs do not reach both ends of the clamp"
    eye = torch.eye(3, 4, device="cuda")
    assert _bits_equal(r3dgs_exposure.apply_exposure(dv(x), eye if len(shape) == 3 else eye.expand(B, 3, 4).contiguous()), dv(x))
    if len(shape) == 4:   # one exposure for the whole batch
        assert _bits_equal(r3dgs_exposure.apply_exposure(dv(x), dv(E[0]))[0], got[0])


def test_training_step_end_to_end():
    """160 x 112 / 3000: render(...) -> exposed_l1_dssim with a table entry and a mask -> backward, against the same step
    written as the official torch lines in front of r3dgs_loss.l1_dssim: model gradients within 1e-4 * max, the table's
    gradient within 1e-4 * max and zero outside the used row."""
    import r3dgs_exposure
    import r3dgs_loss
    import r3dgs_render
    from tests import aux_ref as ar
    from tests.test_aux_grad_gpu import BG, Model
    from tests.test_feature_maps_gpu import PIPE, view_of
    kw = dict(P=3000, W=160, H=112, f=130.0, cam_seed=4, gseed=31, degree_mode="mixed", scale_mu=0.05)
    cam, g, _ = ar.make_scene(kw)
    H, W = kw["H"], kw["W"]
    pc, view, bg = Model(g), view_of(cam, H, W), dv(BG)
    _, gt, m = ref.inputs((3, H, W), seed=91)
    gt, m = dv(gt), dv(m[0])
    start = dv(ref.exposure_guess(4, seed=9))
    used = 2

    def step(fused):
        table = r3dgs_exposure.ExposureTable(4).cuda()
        with torch.no_grad():
            table.exposure.copy_(start)
        for t in pc.leaves():
            t.grad = None
        out = r3dgs_render.render(view, pc, PIPE, bg)
        image, E = out["render"], table[used]
        if fused:
            loss = r3dgs_exposure.exposed_l1_dssim(image, gt, E, m, False, LAM)[0]
        else:
            image = torch.matmul(image.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
            image = image * m
            loss = r3dgs_loss.l1_dssim(image, gt, LAM)[0]
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), [t.grad.clone() for t in pc.leaves()] + [out["viewspace_points"].grad.clone(), table.exposure.grad.clone()]

    loss_f, fused = step(True)
    loss_t, lines = step(False)
    assert abs(loss_f - loss_t) <= 1e-6
    worst = 0.0
    for a, b in zip(fused, lines):
        top = b.abs().max().item()
        assert top > 0
        worst = max(worst, (a - b).abs().max().item() / top)
    print(f"exposure loss end to end 160x112 / 3000: loss {loss_f:.6f} (torch lines {loss_t:.6f}), worst gradient difference {worst:.2e} of max (bar 1e-4)")
    assert worst <= 1e-4
    dE = fused[-1]
    assert dE[used].abs().min() > 0 and not dE[[0, 1, 3]].any(), "the table's gradient is non-zero in the used row alone"
