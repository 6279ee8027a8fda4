"""Times the 3DGS-MCMC calls (include/r3dgs_mcmc.h, csrc/mcmc.hip, reduced-3dgs_amd/r3dgs_mcmc.py) against the same updates
written as torch lines, in alternating blocks, and appends one JSON line per size to profiles/mcmc_bench.jsonl.

    python tools/mcmc_bench.py [--sizes 500000 2000000] [--blocks 6] [--per-block 20]

Per block and size:
  * `noise` / `noise_torch`: inject_noise with a given noise tensor, and the torch lines below (build_rotation, the [P,3,3]
    covariance, the gate, the bmm), between two events;
  * `refine` / `refine_torch`: relocate + add_new on a fresh copy of the model (a tenth of it dead, the cap far away), and their
    torch restatement (multinomial, bincount, boolean-mask indexing, cat; its host waits included), timed with the wall clock
    around a synchronize because the torch arm waits on the host.  The copy of the model is made outside the timed region.
Medians over the blocks, with every block's figure beside them.  No speed bar is set.  Needs an MI355X."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch   # noqa: E402

import r3dgs_mcmc as mc   # noqa: E402
from diff_gaussian_rasterization import _C   # noqa: E402

GROUPS = (("xyz", "_xyz", (3,)), ("f_dc", "_features_dc", (1, 3)), ("f_rest", "_features_rest", (15, 3)),
          ("opacity", "_opacity", (1,)), ("scaling", "_scaling", (3,)), ("rotation", "_rotation", (4,)))


def make_model(P, gen):
    pc = types.SimpleNamespace()
    groups = []
    for name, attr, shape in GROUPS:
        t = torch.randn((P,) + shape, device="cuda", generator=gen)
        if name == "opacity":
            t = t * 2.0 - 1.0
            t[::10] = -7.0   # a tenth of the model is dead
        if name == "scaling":
            t = t * 0.5 - 4.0
        p = torch.nn.Parameter(t.contiguous())
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc._degrees = torch.full((P, 1), 3, dtype=torch.int32, device="cuda")
    pc.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in groups:
        p = g["params"][0]
        pc.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    return pc


def clone_model(src):
    pc = types.SimpleNamespace()
    groups = []
    for name, attr, _ in GROUPS:
        p = torch.nn.Parameter(getattr(src, attr).detach().clone())
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc._degrees = src._degrees.clone()
    pc.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in groups:
        p = g["params"][0]
        pc.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    return pc


# ---- the same updates as torch lines -----------------------------------------------------------------------------------------

def build_rotation(r):
    q = r / torch.norm(r, dim=1, keepdim=True).clamp_min(1e-12)
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


@torch.no_grad()
def noise_torch(pc, scale, noise):
    L = build_rotation(pc._rotation) * torch.exp(pc._scaling)[:, None, :]
    cov = L @ L.transpose(1, 2)
    gate = torch.sigmoid(100.0 * ((1 - torch.sigmoid(pc._opacity)) - 0.995))
    pc._xyz.add_(torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1) * gate * scale)


BINOM = torch.tensor([[float(math.comb(n, k)) for k in range(51)] for n in range(51)], dtype=torch.float64)


def new_values_torch(opacity, scaling, ratio, binom, min_opacity=0.005):
    o = torch.sigmoid(opacity).double().squeeze(-1)
    N = ratio.clamp(max=51)
    o_new = 1 - (1 - o) ** (1.0 / N)
    D = torch.zeros_like(o)
    for i in range(1, int(N.max()) + 1):   # a host wait, as the method's torch code has
        for k in range(i):
            term = binom[i - 1, k] * (-1) ** k * o_new ** (k + 1) / (k + 1) ** 0.5
            D += torch.where(N >= i, term, torch.zeros_like(term))
    s_new = (o / D)[:, None] * torch.exp(scaling).double()
    o_new = o_new.clamp(min_opacity, 1 - 2.0 ** -23)
    return torch.log(o_new / (1 - o_new)).float()[:, None], torch.log(s_new).float()


@torch.no_grad()
def refine_torch(pc, cap_max, gen, binom):
    P = pc._xyz.shape[0]
    # relocate
    w = torch.sigmoid(pc._opacity).squeeze(-1)
    dead = w <= 0.005
    dead_idx, alive_idx = dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]
    if dead_idx.numel() and alive_idx.numel():
        sampled = alive_idx[torch.multinomial(w[alive_idx], dead_idx.numel(), replacement=True, generator=gen)]
        ratio = 1 + torch.bincount(sampled, minlength=P)
        src = sampled.unique()
        op, sc = new_values_torch(pc._opacity[src], pc._scaling[src], ratio[src], binom)
        pc._opacity[src], pc._scaling[src] = op, sc
        for _, attr, _ in GROUPS:
            p = getattr(pc, attr)
            p[dead_idx] = p[sampled]
            st = pc.optimizer.state[p]
            st["exp_avg"][src] = 0
            st["exp_avg_sq"][src] = 0
        pc._degrees[dead_idx] = pc._degrees[sampled]
    # grow
    n_new = max(0, min(cap_max, int(1.05 * P)) - P)
    if n_new:
        w = torch.sigmoid(pc._opacity).squeeze(-1)
        sampled = torch.multinomial(w, n_new, replacement=True, generator=gen)
        ratio = 1 + torch.bincount(sampled, minlength=P)
        src = sampled.unique()
        op, sc = new_values_torch(pc._opacity[src], pc._scaling[src], ratio[src], binom)
        pc._opacity[src], pc._scaling[src] = op, sc
        for group in pc.optimizer.param_groups:
            old = group["params"][0]
            st = pc.optimizer.state.pop(old)
            p = torch.nn.Parameter(torch.cat([old.detach(), old.detach()[sampled]], dim=0))
            st["exp_avg"] = torch.cat([st["exp_avg"], torch.zeros_like(p[P:])], dim=0)
            st["exp_avg_sq"] = torch.cat([st["exp_avg_sq"], torch.zeros_like(p[P:])], dim=0)
            group["params"][0] = p
            pc.optimizer.state[p] = st
            setattr(pc, dict((n, a) for n, a, _ in GROUPS)[group["name"]], p)
        pc._degrees = torch.cat([pc._degrees, pc._degrees[sampled]], dim=0)


def refine_hip(pc, cap_max, gen):
    mc.relocate(pc, 0.005, generator=gen)
    mc.add_new(pc, cap_max, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500_000, 2_000_000])
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--refine-per-block", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_bench.jsonl"))
    args = ap.parse_args()
    binom = BINOM.cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for P in args.sizes:
        gen = torch.Generator(device="cuda").manual_seed(P)
        base = make_model(P, gen)
        noise = torch.randn((P, 3), device="cuda", generator=gen)
        scale = 5e5 * 1.6e-4
        a, b = clone_model(base), clone_model(base)
        mc.inject_noise(a, scale, noise=noise)
        noise_torch(b, scale, noise)
        moved = (a._xyz - base._xyz).detach()
        agree = float(((a._xyz - b._xyz).detach().abs().max() / moved.abs().max().clamp_min(1e-30)))
        arms = dict(noise=lambda pc: mc.inject_noise(pc, scale, noise=noise), noise_torch=lambda pc: noise_torch(pc, scale, noise))
        refine = dict(refine=lambda pc: refine_hip(pc, 10 * P, gen), refine_torch=lambda pc: refine_torch(pc, 10 * P, gen, binom))
        for fn in refine.values():   # warm-up
            fn(clone_model(base))
        ms = {k: [] for k in (*arms, *refine)}
        for _ in range(args.blocks):
            for name, fn in arms.items():
                pc = clone_model(base)
                fn(pc)
                e0.record()
                for _ in range(args.per_block):
                    fn(pc)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.per_block)
            for name, fn in refine.items():
                took = 0.0
                for _ in range(args.refine_per_block):
                    pc = clone_model(base)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(pc)
                    torch.cuda.synchronize()
                    took += time.perf_counter() - t0
                ms[name].append(1e3 * took / args.refine_per_block)
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = dict(tool="mcmc_bench", P=P, blocks=args.blocks, per_block=args.per_block, refine_per_block=args.refine_per_block,
                   **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                   **{f"{k}_ms_blocks": [round(x, 4) for x in v] for k, v in ms.items()},
                   noise_over_torch=round(med["noise"] / med["noise_torch"], 6),
                   refine_over_torch=round(med["refine"] / med["refine_torch"], 3),
                   noise_bytes=68 * P, noise_gb_per_s=round(68 * P / med["noise"] / 1e6, 1),
                   noise_against_torch_rel=agree,
                   note="noise: events around per_block back-to-back calls on the same tensors (they fit the last-level cache: a cache-warm "
                        "figure); refine: wall clock around relocate + add_new on a fresh "
                        "copy (a tenth dead, 5 % growth), synchronize included, the copy outside",
                   library=_C.version(), device=torch.cuda.get_device_name(0), time=time.strftime("%Y-%m-%d %H:%M:%S"))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row))


if __name__ == "__main__":
    main()
