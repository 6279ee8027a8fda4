"""Numpy restatement of the per-iteration training statistics (include/r3dgs_trainstats.h), written from the four lines of the
reference's loop they replace, with vis = radii > 0:

    train.py:105-106           Lalpha_regul = gaussians.get_opacity[vis].abs().mean()             get_opacity = sigmoid(_opacity)
    train.py:113               gaussians._features_rest.detach()[vis].abs().mean()
    train.py:134               max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis])
    gaussian_model.py:693-695  xyz_gradient_accum += norm(viewspace.grad[:, :2]);  denom += vis

The means and the sigmoid are evaluated in float64 (the kernels sum in double and round once); the accumulator update rounds
in float32 exactly where csrc/stats_math.h does, so that it can be compared bit for bit.  Shared by tests/test_train_stats_cpu.py
and tests/test_train_stats_gpu.py; tools/train_stats_bench.py takes the byte count from it.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24   # unit roundoff of float32: one correctly rounded operation has relative error <= U

# Documented accuracy of expf: 1 ulp, for the host (glibc's "Known Maximum Errors in Math Functions", x86_64: expf 1) and for
# the device (HIP math API, single precision: expf 1 ulp).  1 ulp is at most 2^-23 = 2 U relative.
EXPF_REL = 2 * U

# stats_sigmoid(x) = 1 / (1 + e), e = expf(-x).  d ln s / d ln e = -e / (1 + e), magnitude < 1, so e's error enters at most
# once; then one rounding for the add and one for the divide: 2 U + U + U.  Second-order terms: (1 + 2U)(1 + U)^2 - 1 < 4U + 8U^2.
SIGMOID_REL = EXPF_REL + 2 * U + 8 * U * U

# stats_sigmoid_grad(x) = t / (1 + t)^2, t = expf(-|x|) <= 1.  d ln / d ln t = (1 - t) / (1 + t), magnitude <= 1: 2 U; the add's
# rounding enters twice (the square): 2 U; the multiply and the divide: U each.  6 U, second order < 32 U^2.
SIGMOID_GRAD_REL = EXPF_REL + 4 * U + 32 * U * U

# alpha_regul_term(x, scale) = stats_sigmoid_grad(x) * scale: one more rounding, the multiply.
ALPHA_TERM_REL = SIGMOID_GRAD_REL + U

# |x| up to which the bounds hold: beyond it expf(-|x|) leaves float32's normal range (e^-87.3) and expf(x) its finite one
# (e^88.7), where a relative bound means nothing.  Raw opacities of a trained model lie within a few tens.
SIGMOID_DOMAIN = 80.0


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def sigmoid_grad64(x):
    """s (1 - s) without the cancellation: t / (1 + t)^2 with t = exp(-|x|)."""
    t = np.exp(-np.abs(np.asarray(x, np.float64)))
    return t / ((1.0 + t) * (1.0 + t))


def visible_means(radii, opacity=None, features_rest=None):
    """-> dict(mask bool[P], n int, alpha_mean float64 or None, sh_abs_mean float64 or None); empty means are NaN."""
    mask = np.asarray(radii) > 0
    n = int(mask.sum())
    out = {"mask": mask, "n": n, "alpha_mean": None, "sh_abs_mean": None}
    with np.errstate(invalid="ignore", divide="ignore"):
        if opacity is not None:
            s = sigmoid64(np.asarray(opacity).reshape(-1))[mask]
            out["alpha_mean"] = np.float64(s.sum()) / np.float64(n)
        if features_rest is not None:
            rows = np.abs(np.asarray(features_rest, np.float64)[mask])
            out["sh_abs_mean"] = np.float64(rows.sum()) / np.float64(rows.size)
    return out


def alpha_regul_increment(radii, opacity, upstream, n):
    """What alpha_regul_backward adds to dL_dopacity, in float64: vis * sigmoid'(x) * scale.  scale = upstream / n is the ONE
    float32 divide the kernel makes per thread (both operands are exact float32 values), restated in float32."""
    mask = np.asarray(radii) > 0
    if n == 0:
        return np.zeros(mask.shape, np.float64)
    scale = np.float64(F32(upstream) / F32(n))
    return np.where(mask, sigmoid_grad64(np.asarray(opacity).reshape(-1)) * scale, 0.0)


def densification_stats(viewspace_grad, radii, xyz_gradient_accum, denom, max_radii2D):
    """-> (xyz_gradient_accum', denom', max_radii2D') as float32 arrays of the inputs' shapes; every operation is a float32
    numpy operation (correctly rounded), in stats_math.h's order: gx gx, gy gy, their sum, the square root, the add."""
    vg = np.asarray(viewspace_grad, F32)
    r = np.asarray(radii)
    vis = r > 0
    gx, gy = vg[:, 0], vg[:, 1]
    norm = np.sqrt(gx * gx + gy * gy)
    assert norm.dtype == F32
    acc = np.asarray(xyz_gradient_accum, F32).reshape(-1) + np.where(vis, norm, F32(0))
    den = np.asarray(denom, F32).reshape(-1) + np.where(vis, F32(1), F32(0))
    old = np.asarray(max_radii2D, F32).reshape(-1)
    mx = np.where(vis, np.maximum(old, r.astype(F32)), old)
    return (acc.astype(F32).reshape(np.shape(xyz_gradient_accum)), den.astype(F32).reshape(np.shape(denom)),
            mx.astype(F32).reshape(np.shape(max_radii2D)))


def visible_means_bytes(P, M, n_visible):
    """The bytes visible_means has to move: the visible rows of features_rest, plus radii, opacity and the mask byte per
    Gaussian -- 8 P for radii and opacity, as the roof is stated (tools/train_stats_bench.py)."""
    return n_visible * 12 * (M - 1) + 8 * P
