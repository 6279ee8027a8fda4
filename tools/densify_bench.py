"""Cost of one densification call (scene/gaussian_model.py:670-682): r3dgs_densify.densify_and_prune (csrc/densify.hip) against
the reference's torch lines restated here on the same device tensors (cat, cat, mask-index, mask-index over every parameter,
both Adam moments, _degrees and the accumulators; `.sum().item()` twice; empty_cache()).  One JSON line per size, appended to
--out (default profiles/densify_bench.jsonl).

    python tools/densify_bench.py [--sizes 500000 2000000] [--rounds 5] [--timeout 300] [--out FILE]

Each size runs in a child process of its own under --timeout seconds, and the tool stops at the first one that fails.  Both
forms run in that process in alternating blocks, after a warm-up of each; every repetition starts from a fresh copy of the same
model (the copy is outside the timed window), roughly 5 % cloned, 5 % split and 3 % pruned.  Timed by the host clock around
the call and a synchronise: the torch form's host waits are part of what it costs.  state_bytes: one read and one write of
the state (tests/densify_ref.state_bytes), what the fused call moves.  The GPU is required; there is no CPU fallback."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_TBS = 6.3
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY = 5.0, 0.01, 0.0002, 0.005
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"))


def make_state(P, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)

    def rand(*shape):
        return torch.rand(shape, generator=g, device=dev)
    hot, small, low = rand(P) < 0.10, rand(P) < 0.5, rand(P) < 0.03
    s = {"xyz": torch.randn((P, 3), generator=g, device=dev), "f_dc": torch.randn((P, 1, 3), generator=g, device=dev),
         "f_rest": 0.1 * torch.randn((P, 15, 3), generator=g, device=dev),
         "opacity": torch.where(low, -8.0, 2.0)[:, None] + 0.1 * rand(P, 1),
         "scaling": torch.where(small, -5.0, -2.0)[:, None] + 0.3 * rand(P, 3), "rotation": torch.randn((P, 4), generator=g, device=dev)}
    s["degrees"] = torch.randint(0, 4, (P, 1), generator=g, device=dev, dtype=torch.int32)
    s["denom"] = torch.full((P, 1), 10.0, device=dev)
    s["xyz_gradient_accum"] = torch.where(hot, 10 * 5e-4, 10 * 1e-5)[:, None].contiguous()
    s["max_radii2D"] = 10 * rand(P)
    s["moments"] = {n: (1e-3 * torch.randn_like(s[n]), 1e-6 * torch.rand_like(s[n])) for n, _ in GROUPS}
    return s


def make_model(s):
    import r3dgs_optim
    pc = types.SimpleNamespace(percent_dense=PERCENT_DENSE)
    groups = []
    for name, attr in GROUPS:
        p = torch.nn.Parameter(s[name].clone())
        setattr(pc, attr, p)
        groups.append({"params": [p], "lr": 1e-3, "name": name})
    pc.optimizer = r3dgs_optim.Adam(groups, lr=0.0, eps=1e-15)
    for grp in groups:
        m, v = s["moments"][grp["name"]]
        pc.optimizer.state[grp["params"][0]] = {"step": torch.tensor(100.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    pc._degrees = s["degrees"].clone()
    for key in ("xyz_gradient_accum", "denom", "max_radii2D"):
        setattr(pc, key, s[key].clone())
    return pc


# ---- the reference's lines, on a model of this tool's shape --------------------------------------------------------------------
def densify_torch(pc, max_grad, min_opacity, extent, max_screen_size):
    def cat(new, new_degrees):                                                               # :570-620
        for group in pc.optimizer.param_groups:
            old, ext = group["params"][0], new[group["name"]]
            state = pc.optimizer.state.get(old, None)
            if state is not None:
                state["exp_avg"] = torch.cat((state["exp_avg"], torch.zeros_like(ext)), dim=0)
                state["exp_avg_sq"] = torch.cat((state["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
                del pc.optimizer.state[old]
            group["params"][0] = torch.nn.Parameter(torch.cat((old, ext), dim=0).requires_grad_(True))
            if state is not None:
                pc.optimizer.state[group["params"][0]] = state
            setattr(pc, dict(GROUPS)[group["name"]], group["params"][0])
        pc._degrees = torch.cat((pc._degrees, new_degrees), dim=0)
        n = pc._xyz.shape[0]
        pc.xyz_gradient_accum = torch.zeros((n, 1), device="cuda")
        pc.density_gradient_accum = torch.zeros((n, 1), device="cuda")
        pc.denom = torch.zeros((n, 1), device="cuda")
        pc.max_radii2D = torch.zeros((n), device="cuda")

    def prune_points(mask):                                                                  # :502-522, :553-568
        keep = ~mask
        for group in pc.optimizer.param_groups:
            old = group["params"][0]
            state = pc.optimizer.state.get(old, None)
            if state is not None:
                state["exp_avg"], state["exp_avg_sq"] = state["exp_avg"][keep], state["exp_avg_sq"][keep]
                del pc.optimizer.state[old]
            group["params"][0] = torch.nn.Parameter(old[keep].requires_grad_(True))
            if state is not None:
                pc.optimizer.state[group["params"][0]] = state
            setattr(pc, dict(GROUPS)[group["name"]], group["params"][0])
        pc._degrees = pc._degrees[keep]
        pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = pc.xyz_gradient_accum[keep], pc.denom[keep], pc.max_radii2D[keep]

    with torch.no_grad():
        grads = pc.xyz_gradient_accum / pc.denom                                             # :671-672
        grads[grads.isnan()] = 0.0
        sel = grads.squeeze() >= max_grad                                                    # :651-668
        sel = torch.logical_and(sel, torch.max(torch.exp(pc._scaling), dim=1).values <= pc.percent_dense * extent)
        n_cloned = sel.sum().item()
        cat({name: getattr(pc, attr)[sel] for name, attr in GROUPS}, pc._degrees[sel])
        n = pc._xyz.shape[0]                                                                 # :622-649
        padded = torch.zeros((n), device="cuda")
        padded[:grads.shape[0]] = grads.squeeze()
        sel = padded >= max_grad
        sel = torch.logical_and(sel, torch.max(torch.exp(pc._scaling), dim=1).values > pc.percent_dense * extent)
        n_split = sel.sum().item()
        stds = torch.exp(pc._scaling)[sel].repeat(2, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device="cuda"), std=stds)
        q = pc._rotation[sel]
        q = q / torch.sqrt((q * q).sum(dim=1))[:, None]
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                         1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                         1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3).repeat(2, 1, 1)
        new = {name: getattr(pc, attr)[sel].repeat(2, *([1] * (getattr(pc, attr).dim() - 1))) for name, attr in GROUPS}
        new["xyz"] = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + pc._xyz[sel].repeat(2, 1)
        new["scaling"] = torch.log(torch.exp(pc._scaling)[sel].repeat(2, 1) / (0.8 * 2))
        cat(new, pc._degrees[sel].repeat(2, 1))
        prune_points(torch.cat((sel, torch.zeros(2 * sel.sum(), device="cuda", dtype=bool))))
        mask = (torch.sigmoid(pc._opacity) < min_opacity).squeeze()                          # :684-691
        if max_screen_size:
            mask = torch.logical_or(torch.logical_or(mask, pc.max_radii2D > max_screen_size),
                                    torch.exp(pc._scaling).max(dim=1).values > 0.1 * extent)
        n_pruned = mask.sum()
        prune_points(mask)
        torch.cuda.empty_cache()
    return n_cloned, n_split, int(n_pruned)


def densify_hip(pc, max_grad, min_opacity, extent, max_screen_size):
    import r3dgs_densify
    stats = {}
    r3dgs_densify.densify_and_prune(pc, max_grad, min_opacity, extent, max_screen_size, stats)
    return stats["n_points_cloned"], stats["n_points_split"], stats["n_points_pruned"]


FORMS = {"torch": densify_torch, "hip": densify_hip}


def bench(P, rounds):
    from tests import densify_ref
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = make_state(P, dev)
    ms, counts, rows = {k: [] for k in FORMS}, {}, {}

    def once(form, record):
        pc = make_model(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts[form] = FORMS[form](pc, MAX_GRAD, MIN_OPACITY, EXTENT, 20)
        torch.cuda.synchronize()
        if record:
            ms[form].append((time.perf_counter() - t0) * 1e3)
        rows[form] = pc._xyz.shape[0]
    for form in FORMS:
        once(form, False)
        once(form, False)
    for _ in range(rounds):
        for form in FORMS:
            once(form, True)
    assert counts["torch"] == counts["hip"] and rows["torch"] == rows["hip"], (counts, rows)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    nbytes = densify_ref.state_bytes(P, 16) + densify_ref.state_bytes(rows["hip"], 16)
    return {"metric": "densify", "gaussians": P, "gaussians_after": rows["hip"], "cloned_split_pruned": list(counts["hip"]),
            "densify_ms": med, "densify_ms_all": ms, "speedup": med["torch"] / med["hip"], "state_bytes": nbytes,
            "roof_ms": nbytes / (HBM_TBS * 1e12) * 1e3, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[500_000, 2_000_000])
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two forms")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.jsonl"))
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        if not torch.cuda.is_available():
            raise SystemExit("densify_bench.py needs a GPU")
        print(json.dumps(bench(args.one, args.rounds)), flush=True)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for P in args.sizes:   # a fresh process per size, under its own time limit; nothing is started after a failure
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(P), "--rounds", str(args.rounds)],
                           capture_output=True, text=True, timeout=args.timeout)
        if r.returncode != 0:
            raise SystemExit(f"densify_bench.py: {P} Gaussians failed (exit status {r.returncode}); stopping\n{r.stderr[-2000:]}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
