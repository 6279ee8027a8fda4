"""Where does torch's ROCm build round in its default (foreach) Adam step?  Runs one torch.optim.Adam step on the GPU
(default path, and fused=True) on crafted fp32 inputs -- wide magnitudes, zeros, tiny v, huge g; steps 1 to 10^4; lerp weights
below and above 0.5 -- and compares it bit for bit with the sixteen float32 restatements
{lerp, addcmul, addcdiv: one fma or a rounded product and sum} x {divide by bc2_sqrt or multiply by its reciprocal}.
csrc/adam_math.h implements the one variant that matches.  Prints one line per variant and form.

    python tools/adam_rounding_sweep.py"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.adam_ref import F32, fma32, host_scalars  # noqa: E402

CASES = [(1, 1.6e-4, 0.9, 0.999, 1e-15), (10, 0.0025, 0.9, 0.999, 1e-15), (10000, 0.05, 0.9, 0.999, 1e-15),
         (3, 0.005, 0.9, 0.999, 1e-8), (7, 0.001, 0.3, 0.99, 1e-8), (2, 0.01, 0.7, 0.5, 1e-6)]


def inputs(rng, n):
    p = rng.standard_normal(n).astype(F32) * F32(3)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 3, n)).astype(F32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 2, n)).astype(F32)
    v = (10.0 ** rng.uniform(-30, 4, n)).astype(F32)
    g[:64] = 0
    m[64:128] = 0
    v[128:192] = 0
    g[192:256] = 1e18
    v[256:320] = 1e-38
    return p, g, m, v


def torch_step(p, g, m, v, case, fused):
    step, lr, b1, b2, eps = case
    t = torch.nn.Parameter(torch.from_numpy(p).cuda())
    opt = torch.optim.Adam([t], lr=lr, betas=(b1, b2), eps=eps, **({"fused": True} if fused else {}))
    t.grad = torch.from_numpy(g).cuda()
    st = opt.state[t]
    st["step"] = torch.tensor(float(step - 1), device="cuda" if fused else "cpu")
    st["exp_avg"] = torch.from_numpy(m.copy()).cuda()
    st["exp_avg_sq"] = torch.from_numpy(v.copy()).cuda()
    opt.step()
    return t.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


def variant(p, g, m, v, s, lerp_fma, addcmul_fma, recip, addcdiv_fma):
    with np.errstate(all="ignore"):
        w, dg = s["w1"], g - m
        if w < F32(0.5):
            m1 = fma32(w, dg, m) if lerp_fma else m + w * dg
        else:
            om = F32(1) - w
            m1 = fma32(-dg, om, g) if lerp_fma else g - dg * om
        v1, gg = v * s["beta2"], g * g
        v1 = fma32(s["w2"], gg, v1) if addcmul_fma else v1 + s["w2"] * gg
        sq = np.sqrt(v1)
        sq = sq * (F32(1) / s["bc2_sqrt"]) if recip else sq / s["bc2_sqrt"]
        q = m1 / (sq + s["eps"])
        p1 = fma32(s["step_size"], q, p) if addcdiv_fma else p + s["step_size"] * q
    return p1, m1, v1


def main():
    rng = np.random.default_rng(7)
    data = [inputs(rng, 1 << 16) for _ in CASES]
    print(f"torch {torch.__version__} hip {torch.version.hip}; {len(CASES)} cases x {1 << 16} elements")
    for fused in (False, True):
        ref = [torch_step(*d, c, fused) for d, c in zip(data, CASES)]
        for flags in itertools.product((0, 1), repeat=4):
            mism = [0, 0, 0]
            for d, c, r in zip(data, CASES, ref):
                got = variant(*d, host_scalars(c[1], c[2], c[3], c[4], c[0]), *flags)
                for k in range(3):
                    mism[k] += int((got[k].view(np.uint32) != r[k].view(np.uint32)).sum())
            verdict = "MATCH" if not any(mism) else f"differ p {mism[0]} m {mism[1]} v {mism[2]}"
            print(f"{'fused=True' if fused else 'foreach   '} lerp_fma={flags[0]} addcmul_fma={flags[1]} "
                  f"div_by_reciprocal={flags[2]} addcdiv_fma={flags[3]}: {verdict}")


if __name__ == "__main__":
    main()
