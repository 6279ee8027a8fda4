"""Scenes shared by tests/test_camera_grad_cpu.py and tests/test_camera_grad_gpu.py (a plain helper module, not a conftest).
The seeds are chosen so that the oracle alone flags at most 1e-3 of each scene's pixels as threshold-ambiguous
(test_camera_grad_cpu.py asserts it)."""
import numpy as np

import synth_scene as ss
from tests import camera_cases as cc

BG = np.array([0.1, 0.3, 0.2], np.float32)
# the kernel-alone scenes: 96x64, fx != fy, a small rigid motion, about a third of the Gaussians culled, mixed degrees
KERNEL_SIZES = (37, 64, 3001)
KERNEL_SEEDS = {37: 1, 64: 1, 3001: 2}
GAUGE = dict(P=20_000, W=400, H=400, seed=1)
POSE = dict(P=400, W=64, H=48, seed=4, offset=(0.02, -0.03, 0.025, 0.03, -0.02, 0.04))   # rotation vector, translation


# ---- measured figures, written once: tests/test_camera_grad_cpu.py reproduces each, tests/test_camera_grad_gpu.py uses them ----
# What the fp32 forward state alone is worth for the 35 sums, as a fraction of each tensor's largest entry: the reference fed
# orc.backward_f64 on the fp32 state, against end-to-end fp64 autograd, at worst over the two scenes of the end-to-end GPU test
# (viewmatrix 2.3e-6, projmatrix 6.44e-6, campos 1.9e-6).  Under a quarter of the gradient bar 1e-4, so that test keeps 1e-4.
STATE_ROUNDING = 6.44e-6
# |sum_i dL_dmeans3D_i - (V[:3,:] gV[3,:] + F[:3,:] gF[3,:] - g_campos)| of the CPU oracle's own fp32 gradients on the gauge
# scene, as a fraction of the left side's largest component.  The gauge test on the GPU allows four times this.
GAUGE_RESIDUAL = 7.605e-7
# the pose-recovery loop: Adam steps and rate, and final / initial loss of the fp64 run through oracle/torch_ref
POSE_LR, POSE_STEPS, POSE_RATIO_FP64 = 1.5e-3, 40, 0.1021


def kernel_scene(P):
    """-> (camera, Gaussians) at 96x64."""
    rng = np.random.default_rng(50 + P)
    cam = ss.Camera(96, 64, 80.0, 62.0, ss.rot_xyz(*rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.3, 0.3, 3))
    # (drawn for the camera's intrinsics in the world frame: the small rigid motion keeps the cloud in view)
    return cam, ss.make_gaussians(P, cam, seed=KERNEL_SEEDS[P], degree_mode="mixed", scale_mu=0.05, behind_frac=0.2)


def portrait_scene():
    """The portrait, far-rotated camera of tests/camera_cases.py at its gpu size (117x203), 1500 Gaussians."""
    return cc.cloud("portrait_far", "gpu", 1500, 6)


def gauge_scene():
    kw = GAUGE
    cam = ss.make_camera(kw["W"], kw["H"], 300.0, seed=2)
    return cam, ss.make_gaussians(kw["P"], cam, seed=kw["seed"], degree_mode="mixed", scale_mu=0.02)


def pose_scene():
    kw = POSE
    cam = ss.Camera(kw["W"], kw["H"], 55.0, 50.0, ss.rot_xyz(0.03, -0.05, 0.02), (0.1, -0.05, 0.2))
    return cam, ss.make_gaussians(kw["P"], cam, seed=kw["seed"], degree_mode="mixed", scale_mu=0.08, behind_frac=0.0)


def oracle_forward(cam, g, want_ambig=True):
    from oracle import oracle as orc
    return orc.forward(BG, g["means3D"], None, g["opacity"], g["scales"], g["rotations"], 1.0, None, cam.world_view_transform,
                       cam.full_proj_transform, cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, g["sh"], g["degrees"],
                       cam.camera_center, want_ambig=want_ambig)


def upstream(cam, ambig, seed):
    """Seeded dL/dimage of unit scale, zero on the oracle's ambiguous pixels."""
    W, H = cam.image_width, cam.image_height
    dl = ss.upstream_grad(W, H, seed=seed) * W * H
    dl.reshape(3, -1)[:, np.asarray(ambig).reshape(-1) != 0] = 0.0
    return dl


def pose_target_and_start():
    """-> (camera, Gaussians, the true world_view_transform as float64 [4,4] (transposed), the start true @ exp(-offset)^T: a
    RefinedCamera built on the start reaches the true pose at xi = offset)."""
    import torch

    from r3dgs_camera import se3_exp
    cam, g = pose_scene()
    true = cam.world_view_transform.astype(np.float64)
    start = true @ se3_exp(-torch.tensor(POSE["offset"], dtype=torch.float64)).t().numpy()
    return cam, g, true, start
