"""GPU tests (-m gpu) of the codebook-space fine-tune: r3dgs_quantised_codebook_grad through both bindings against a float64
sum over the slot enumeration (tests/quant_grad_ref.py; the bar is derived from "double accumulation, one rounding" and
nothing is masked), its determinism (two calls, a replayed graph, ctypes == compiled), the autograd route of
r3dgs_render.render for a trainable QuantisedModel against the dense training route of its decode(), commit() / to_ply(), and
a 40-step fine-tune of the codebooks.

Measured on an MI355X (printed by test_fine_tune_of_the_codebooks_lowers_the_loss): see DESIGN.md 15."""
import math
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import synth_scene as ss
from tests import quant_grad_ref as gr
from tests import quant_ref as qr

pytestmark = pytest.mark.gpu
CHUNK = 1024   # asserted against the library's constant in test_the_large_mix_spans_three_chunks
BIG = (CHUNK - 301, CHUNK // 2 + 37, CHUNK - 23, CHUNK - 300)   # 2997: three chunks, the last one partial
SHAPES = {"-".join(map(str, c)): c for c in qr.MIXES + [BIG, (0, 0, 1, 0)]}
PATTERNS = ("random", "equal", "mod256", "ends")
PIPE = NS(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def patterned(counts, pattern):
    """The model of `counts` with its ids rewritten: equal -- every id 7, every book's worst conflict; mod256 -- id i mod
    256 along each id array; ends -- only centres 0 and 255 are named."""
    m = qr.make_model(counts, seed=3 + sum(counts))
    rng = np.random.default_rng(17)
    for k in ("geom_ids", "sh_ids"):
        a = m[k]
        if pattern == "equal":
            a[...] = 7
        elif pattern == "mod256":
            a[...] = (np.arange(a.size) % 256).astype(np.uint8).reshape(a.shape)
        elif pattern == "ends":
            a[...] = (rng.integers(0, 2, a.shape) * 255).astype(np.uint8)
    return m


_cases = {}


def case(shape, pattern):
    """(model arrays, slot rows, gradients, device arguments), computed once per case and shared."""
    key = (shape, pattern)
    if key not in _cases:
        m = patterned(SHAPES[shape], pattern)
        P = sum(m["counts"])
        coeffs, per, cum = qr.tables(m["counts"])
        ids = (_dev(m["geom_ids"]), _dev(m["sh_ids"]), _dev(per), _dev(cum), _dev(coeffs))
        _cases[key] = (m, gr.np_slots(m), gr.make_grads(P, seed=P + len(pattern)), ids)
    return _cases[key]


def run(ids, grads, binding=None):
    from diff_gaussian_rasterization import _C
    was = _C.set_binding(binding) if binding else None
    try:
        out = _C.quantised_codebook_grad(*ids, *(None if grads[n] is None else _dev(grads[n]) for n in gr.TENSORS))
    finally:
        if binding:
            _C.set_binding(was)
    assert out.dtype == torch.float32 and tuple(out.shape) == (20, 256)
    return out.cpu().numpy()


def test_the_large_mix_spans_three_chunks():
    from diff_gaussian_rasterization import _C
    assert CHUNK == _C.QUANTISED_GRAD_CHUNK
    P = sum(BIG)
    assert all(c % 64 for c in BIG) and 2900 <= P <= 3100
    assert -(-P // CHUNK) >= 3 and P % CHUNK != 0 and P <= _C.QUANTISED_GRAD_MAX_GROUPS * CHUNK   # one chunk per group
    assert _C._lib.r3dgs_quantised_codebook_grad_workspace_bytes(P) == -(-P // CHUNK) * 20 * 256 * 8


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_the_float64_sum(shape, pattern):
    m, slots, grads, ids = case(shape, pattern)
    got = run(ids, grads)
    gr.check(got, slots, grads, (shape, pattern))
    if pattern == "ends":   # only centres 0 and 255 are named: the others come back as +0.0 bits
        assert (got.view(np.uint32)[:, 1:255] == 0).all()
    assert np.array_equal(run(ids, grads).view(np.uint32), got.view(np.uint32))   # two calls, the same bits


@pytest.mark.parametrize("shape", ["37-0-150-70", "63-65-1-130", "-".join(map(str, BIG))])
def test_rows_above_the_degree_are_not_read_and_null_is_zero(shape):
    m, slots, grads, ids = case(shape, "random")
    P = sum(m["counts"])
    deg = np.repeat(np.arange(4), m["counts"])
    above = np.broadcast_to(np.arange(15)[None, :, None] >= ((deg + 1) ** 2 - 1)[:, None, None], (P, 15, 3))
    assert above.any()
    zeroed, noisy = dict(grads), dict(grads)
    zeroed["rest"] = np.where(above, np.float32(0), grads["rest"])
    noisy["rest"] = np.where(above, np.float32(1e6) + grads["rest"] * grads["rest"], grads["rest"]).astype(np.float32)
    assert (noisy["rest"][above] != 0).all()
    want = run(ids, zeroed)
    assert np.array_equal(run(ids, noisy).view(np.uint32), want.view(np.uint32))
    gr.check(want, slots, zeroed, (shape, "above the degree"))
    for name in gr.TENSORS:   # a NULL gradient equals a zero tensor
        null = dict(grads, **{name: None})
        zero = dict(grads, **{name: np.zeros_like(grads[name])})
        got = run(ids, null)
        assert np.array_equal(got.view(np.uint32), run(ids, zero).view(np.uint32)), name
        gr.check(got, slots, null, (shape, name, "NULL"))
    none = run(ids, {n: None for n in gr.TENSORS})
    assert (none.view(np.uint32) == 0).all()


@pytest.mark.parametrize("shape", ["37-0-150-70", "-".join(map(str, BIG))])
def test_bindings_agree_and_a_replayed_graph_follows_new_gradients(shape):
    from diff_gaussian_rasterization import _C
    m, slots, grads, ids = case(shape, "random")
    a, b = run(ids, grads, "ctypes"), run(ids, grads, "torch")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    other = gr.make_grads(sum(m["counts"]), seed=99)
    want_other = run(ids, other)
    assert not np.array_equal(want_other, a)
    for binding in ("ctypes", "torch"):
        was = _C.set_binding(binding)
        try:
            static = [_dev(grads[n]) for n in gr.TENSORS]
            _C.quantised_codebook_grad(*ids, *static)   # warm up outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = _C.quantised_codebook_grad(*ids, *static)
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), a.view(np.uint32)), binding
            for t, n in zip(static, gr.TENSORS):
                t.copy_(_dev(other[n]))
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want_other.view(np.uint32)), binding
        finally:
            _C.set_binding(was)


# ---------------------------------------------------------------------------------------------------------- autograd
def view_of(cam):
    return NS(image_height=cam.image_height, image_width=cam.image_width, FoVx=cam.FoVx, FoVy=cam.FoVy,
              world_view_transform=_dev(cam.world_view_transform), full_proj_transform=_dev(cam.full_proj_transform),
              camera_center=_dev(cam.camera_center))


def bg():
    return _dev(np.array([0.1, 0.2, 0.3], np.float32))


def synthetic_model():
    from r3dgs_quantised import QuantisedModel
    m = qr.make_model((37, 0, 150, 70), seed=11, centre=(0.0, 0.0, 4.0), spread=0.8)
    return QuantisedModel(_dev(m["xyz"]), _dev(m["geom_ids"]), _dev(m["sh_ids"]), _dev(m["codebooks"]), m["counts"]), m


def dense_model(qm):
    """decode()'s tensors as the leaves of a model shaped like the reference's GaussianModel."""
    d = qm.decode()
    dm = NS(active_sh_degree=3, max_sh_degree=3, _degrees=d["_degrees"])
    for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(dm, k, d[k].clone().requires_grad_(True))
    return dm


def test_autograd_equals_the_dense_training_route():
    import r3dgs_render
    from r3dgs_loss import l1_loss
    qm, m = synthetic_model()
    view = view_of(ss.make_camera(80, 48, 60.0, 2))
    target = _dev(np.random.default_rng(4).uniform(0, 1, (3, 48, 80)).astype(np.float32))
    dm = dense_model(qm)
    want = r3dgs_render.render(view, dm, PIPE, bg())
    l1_loss(want["render"], target).backward()
    qm.requires_grad_(codebooks=True, xyz=True)
    got = r3dgs_render.render(view, qm, PIPE, bg())
    assert set(got) == set(want) and (got["radii"] > 0).sum() > 50
    assert torch.equal(got["render"], want["render"]) and torch.equal(got["radii"], want["radii"])
    assert torch.equal(got["visibility_filter"], want["visibility_filter"])
    l1_loss(got["render"], target).backward()
    assert torch.equal(qm.xyz_master.grad, dm._xyz.grad) and dm._xyz.grad.abs().sum() > 0
    assert torch.equal(got["viewspace_points"].grad, want["viewspace_points"].grad)
    grads = {n: getattr(dm, k).grad.cpu().numpy() for n, k in zip(gr.TENSORS, ("_features_dc", "_features_rest", "_opacity",
                                                                               "_scaling", "_rotation"))}
    assert all(np.abs(g).sum() > 0 for g in grads.values())
    gr.check(qm.codebooks.grad.cpu().numpy(), gr.np_slots(m), grads, "autograd")
    # codebooks only: the positions are decoded, and nothing asks for their gradient
    qm.commit(half_float=False)
    qm.requires_grad_(codebooks=True, xyz=False)
    first = qm.codebooks
    out = r3dgs_render.render(view, qm, PIPE, bg())
    assert torch.equal(out["render"], want["render"])
    l1_loss(out["render"], target).backward()
    gr.check(first.grad.cpu().numpy(), gr.np_slots(m), grads, "autograd, codebooks only")
    # under no_grad a trainable model takes the inference route
    with torch.no_grad():
        assert r3dgs_render.render(view, qm, PIPE, bg())["viewspace_points"] is None


def test_nothing_else_moved():
    import r3dgs_render
    from diff_gaussian_rasterization import _C
    qm, _ = synthetic_model()
    cam = ss.make_camera(80, 48, 60.0, 2)
    view = view_of(cam)
    out = r3dgs_render.render(view, qm, PIPE, bg())   # grad enabled, nobody asked for gradients: today's route
    assert out["viewspace_points"] is None and not out["render"].requires_grad
    direct = _C.rasterize_gaussians_quantised(bg(), qm.xyz, qm.geom_ids, qm.sh_ids, qm.codebooks, 1.0, view.world_view_transform,
                                              view.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), 48,
                                              80, qm.per_band, qm.cumsum, qm.coeffs, view.camera_center, False, False)
    assert torch.equal(out["render"], direct[1]) and torch.equal(out["radii"], direct[2])
    for model in (qm, synthetic_model()[0].requires_grad_()):
        with pytest.raises(ValueError, match="lambda_sh_sparsity"):
            r3dgs_render.render(view, model, PIPE, bg(), lambda_sh_sparsity=0.1)


def golden_views():
    return [view_of(ss.Camera(80, 48, 60.0, 60.0, None, T))
            for T in ((0.1, -0.05, 4.0), (-0.2, 0.1, 4.2), (0.3, 0.05, 3.8), (0.0, -0.15, 4.5))]


def training_forward_without_grad(qm, view):
    """The training route's kernels on the model's stored values: decode(), then the raw-parameter forward."""
    import r3dgs_render
    d = qm.decode()
    dm = NS(active_sh_degree=3, max_sh_degree=3, **d)
    with torch.no_grad():
        return r3dgs_render.render(view, dm, PIPE, bg())["render"]


@pytest.mark.parametrize("half", [True, False])
def test_commit_and_to_ply_render_the_committed_values(half, golden_dir, tmp_path):
    import r3dgs_optim
    import r3dgs_render
    from r3dgs_loss import l1_loss
    from r3dgs_quantised import QuantisedModel
    name = "quantised_half_P200.ply" if half else "quantised_P200.ply"
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, name), half)
    views = golden_views()
    target = _dev(np.random.default_rng(8).uniform(0, 1, (3, 48, 80)).astype(np.float32))
    before = qm.codebooks.clone(), qm.xyz.clone()
    qm.requires_grad_()
    opt = r3dgs_optim.Adam(qm.parameters(), lr=1e-3, eps=1e-15)
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        l1_loss(r3dgs_render.render(views[step], qm, PIPE, bg())["render"], target).backward()
        opt.step()
    qm.commit()
    assert not torch.equal(qm.codebooks, before[0]) and not qm.trainable and qm.xyz.dtype == before[1].dtype
    assert half or not torch.equal(qm.xyz, before[1])
    if half:
        assert torch.equal(qm.codebooks, qm.codebooks.half().float())
    path = str(tmp_path / "tuned.ply")
    qm.to_ply(path, half)
    copy = QuantisedModel.from_ply(path, half)
    for a, b in zip(qm.arrays(), copy.arrays()):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for view in views[:2]:
        image = r3dgs_render.render(view, qm, PIPE, bg())["render"]
        assert torch.equal(image, training_forward_without_grad(qm, view))
        assert torch.equal(image, r3dgs_render.render(view, copy, PIPE, bg())["render"])


def _fine_tune(golden_dir, views, targets, steps=40):
    import r3dgs_optim
    import r3dgs_render
    from r3dgs_loss import l1_loss
    from r3dgs_quantised import QuantisedModel
    qm = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)

    def summed():
        with torch.no_grad():
            return sum(float(l1_loss(r3dgs_render.render(v, qm, PIPE, bg())["render"], t)) for v, t in zip(views, targets))
    start = summed()
    qm.requires_grad_(codebooks=True, xyz=False)
    opt = r3dgs_optim.Adam(qm.parameters(), lr=5e-3, eps=1e-15)
    for step in range(steps):
        k = step % len(views)
        opt.zero_grad(set_to_none=True)
        l1_loss(r3dgs_render.render(views[k], qm, PIPE, bg())["render"], targets[k]).backward()
        opt.step()
    return start, summed(), qm.codebooks.detach().clone()


def test_fine_tune_of_the_codebooks_lowers_the_loss(golden_dir):
    """Targets: the file's model with its codebooks perturbed by seeded noise, at four cameras; 40 Adam steps on the codebooks
    from the unperturbed file.  The summed L1 afterwards is below the summed L1 before (no ratio is fixed)."""
    import r3dgs_render
    from r3dgs_quantised import QuantisedModel
    views = golden_views()
    teacher = QuantisedModel.from_ply(os.path.join(golden_dir, "quantised_P200.ply"), False)
    noise = torch.from_numpy(np.random.default_rng(21).normal(0, 0.15, (20, 256)).astype(np.float32)).cuda()
    teacher.codebooks = (teacher.codebooks + noise).contiguous()
    with torch.no_grad():
        targets = [r3dgs_render.render(v, teacher, PIPE, bg())["render"].clone() for v in views]
    start, end, books = _fine_tune(golden_dir, views, targets)
    print(f"summed L1 over four views: {start:.6f} before, {end:.6f} after 40 steps")
    assert end < start
    again = _fine_tune(golden_dir, views, targets)
    assert again[0] == start and again[1] == end and torch.equal(again[2].view(torch.int32), books.view(torch.int32))
