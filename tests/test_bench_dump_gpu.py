"""bench.py --dump-outputs end to end: what a plain run writes is the last TIMED step's outputs -- the same image, radii and
gradients as one direct forward + backward of that step's camera through the autograd boundary, on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth_scene as ss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD, CAMERAS, WARMUP, STEPS = "lego_like_300k_800", 4, 2, 4   # last timed step 5 -> camera 1 (bench.cam_index)


def _step(cam_id):
    """One training step of bench.py's train_step() on camera `cam_id`, as the caller sees it."""
    import diff_gaussian_rasterization as dgr
    w = ss.WORKLOADS[WORKLOAD]
    W, H = w["W"], w["H"]
    _, cam0, g = ss.make_workload(WORKLOAD, seed=0)
    cam = cam0 if cam_id == 0 else ss.make_camera(W, H, w["f"], cam_id)

    def dv(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    leaves = {k: dv(g[k]).requires_grad_() for k in ("means3D", "opacity", "scales", "rotations", "sh")}
    rs = dgr.GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, dv(np.zeros(3, np.float32)), 1.0,
                                           dv(cam.world_view_transform), dv(cam.full_proj_transform), 3,
                                           dv(cam.camera_center), False, False)
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True) + 0
    means2D.retain_grad()
    empty = torch.Tensor([])
    color, radii = dgr.rasterize_gaussians(leaves["means3D"], means2D, leaves["sh"], dv(g["degrees"]), empty,
                                           leaves["opacity"], leaves["scales"], leaves["rotations"], empty, rs, 0.0)
    color.backward(dv(ss.upstream_grad(W, H, seed=1)))
    torch.cuda.synchronize()
    out = {"color": color.detach().cpu().numpy(), "radii": radii.float().cpu().numpy(),
           "grad_means2D": means2D.grad.cpu().numpy()}
    out.update({f"grad_{k}": v.grad.cpu().numpy() for k, v in leaves.items()})
    return out


def test_dump_outputs_are_the_last_timed_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", WORKLOAD,
                        "--cameras", str(CAMERAS), "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(d)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) < 64 * 2 ** 20
    assert all(a.dtype == (np.float64 if k == "gaussian_index" else np.float32) for k, a in got.items())
    idx = got.pop("gaussian_index").astype(np.int64)   # 300 k rows do not fit the budget: a sample of them is written
    want = _step((WARMUP + STEPS - 1) % CAMERAS)
    assert set(got) == set(want)
    np.testing.assert_array_equal(got["color"], want["color"])
    for k in set(want) - {"color"}:
        ref = want[k][idx]
        np.testing.assert_allclose(got[k], ref, rtol=1e-6, atol=1e-6 * float(np.abs(ref).max()), err_msg=k)
    other = _step((WARMUP + STEPS - 2) % CAMERAS)   # the step before, another camera: clearly not what was written
    assert np.abs(other["color"] - got["color"]).max() > 1e-2
