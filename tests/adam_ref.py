"""Numpy restatements of one Adam step, shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py.

`step32` rounds to float32 after every operation exactly where reduced-3dgs_amd/csrc/adam_math.h documents a rounding (and
so where torch/optim/adam.py::_multi_tensor_adam's elementwise kernels round, capturable=False): numpy's float32 add, mul,
div and sqrt are IEEE correctly rounded, and `fma32` emulates a fused multiply-add exactly (Python 3.10 has no math.fma).
`host_scalars` computes the per-tensor scalars in Python doubles as torch does.  `step64` is the float64 evaluation of the
same formula, the yardstick of the capturable path."""
import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """float32(a * b + c) with one rounding.  a * b is exact in float64 (24 + 24 bits); s = a * b + c rounded to float64 and
    its exact error e (TwoSum) give the exact sum s + e.  Rounding s to float32 is then the correct rounding of s + e except
    when s sits exactly half-way between two float32 values and e != 0: the tie breaks towards e."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(F32)
        diff = s - r.astype(np.float64)
        toward = np.where(diff > 0, F32(np.inf), F32(-np.inf))
        nb = np.nextafter(r, toward)
        tie = (diff != 0) & (2.0 * np.abs(diff) == np.abs(nb.astype(np.float64) - r.astype(np.float64))) & (e != 0)
        out = np.where(tie & (np.sign(e) == np.sign(diff)), nb, r)
    return np.asarray(out, F32)


def host_scalars(lr, beta1, beta2, eps, step):
    """The per-tensor scalars of one step, as torch computes them in Python doubles (step: the bumped count), each rounded
    to float32 once, as a Python scalar reaches a float32 kernel."""
    step = float(step)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    step_size = (lr / bc1) * -1
    bc2_sqrt = bc2 ** 0.5
    return dict(w1=F32(1 - beta1), beta2=F32(beta2), w2=F32(1 - beta2), bc2_sqrt=F32(bc2_sqrt), eps=F32(eps),
                step_size=F32(step_size))


def step32(p, g, m, v, s):
    """One step in float32, op for op as csrc/adam_math.h (s: host_scalars).  Returns (p, m, v)."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        w = s["w1"]
        if w < F32(0.5):   # lerp(m, g, w): m + w (g - m), one fma
            m1 = fma32(w, g - m, m)
        else:              # g - (g - m)(1 - w), one fma
            m1 = fma32(-(g - m), F32(1) - w, g)
        v1 = v * s["beta2"]
        v1 = fma32(s["w2"], g * g, v1)                 # addcmul: v + w2 (g g), one fma
        d = np.sqrt(v1) / s["bc2_sqrt"] + s["eps"]     # three roundings
        p1 = fma32(s["step_size"], m1 / d, p)          # addcdiv: p + step_size (m / d), one fma
    return p1, m1, v1


def step64(p, g, m, v, lr, beta1, beta2, eps, step):
    """The same step in float64 throughout (bias corrections from the bumped step)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    m1 = m + (1 - beta1) * (g - m)
    v1 = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p1 = p - (lr / bc1) * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
    return p1, m1, v1


# The six parameter groups of scene/gaussian_model.py:210-217 (training_setup): per-Gaussian shape and the initial lr of
# arguments/__init__.py (feature_lr / 20 for f_rest; xyz with spatial_lr_scale 1), 59 floats per Gaussian at degree 3.
GROUPS = (("xyz", (3,), 0.00016), ("f_dc", (1, 3), 0.0025), ("f_rest", (15, 3), 0.0025 / 20.0), ("opacity", (1,), 0.05),
          ("scaling", (3,), 0.005), ("rotation", (4,), 0.001))


def xyz_lr(it, lr_init=0.00016, lr_final=0.0000016, max_steps=30_000):
    """An exponential decay shaped like the reference's xyz schedule, so the lr changes every step."""
    t = min(max(it / max_steps, 0.0), 1.0)
    return float(np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
