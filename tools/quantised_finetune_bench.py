"""Cost of the codebook-space fine-tune of a quantised model (r3dgs_quantised.py, csrc/quant_grad.hip) at the 2 M and 6 M
stand-ins of synth_scene.WORKLOADS.

    python tools/quantised_finetune_bench.py [--iters 10] [--rounds 3] [--workloads garden_like_2M_1600x1062 ...]
                                             [--out profiles/quantised_finetune_bench.jsonl]

Per workload the Gaussians are quantised on the host (per attribute: 256 quantile centres, the nearest one's id), sorted by
degree, and three things are timed between device events, in blocks of --iters calls, --rounds times after a warm-up:
  kernel        _C.quantised_codebook_grad on five random gradient tensors
  index_add     the torch formulation on the same tensors: twenty index_add_ calls over strided columns (float atomics: its
                result changes from run to run); the two legs alternate block by block
  step          a whole fine-tune step: render() of the trainable model, r3dgs_loss.l1_loss, backward, r3dgs_optim.Adam.step
One JSON line per workload, printed and appended to --out: the medians, every block, the bytes the kernel has to read
(236 + 8 + 3 (d+1)^2 per Gaussian) and that over the kernel's time.  The GPU is required; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reduced-3dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import r3dgs_optim  # noqa: E402
import synth_scene as ss  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from r3dgs_loss import l1_loss  # noqa: E402
from r3dgs_quantised import QuantisedModel  # noqa: E402
from r3dgs_render import render  # noqa: E402

DEFAULT = ("garden_like_2M_1600x1062", "train_like_6M_1920x1080")


def timed(body, count):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(count):
        body()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / count


def quantise(x):
    """float array [n, ...] -> (256 centres: its quantiles, uint8 ids of the nearest centre by rank)."""
    flat = x.reshape(-1).astype(np.float32)
    sample = flat if flat.size <= 1 << 20 else flat[:: flat.size >> 20]
    centres = np.quantile(sample, (np.arange(256) + 0.5) / 256).astype(np.float32)
    edges = (centres[1:] + centres[:-1]) / 2
    return centres, np.searchsorted(edges, flat).astype(np.uint8).reshape(x.shape)


def quantised_workload(name):
    w, cam, g = ss.make_workload(name)
    order = np.argsort(g["degrees"].reshape(-1), kind="stable")
    deg = g["degrees"].reshape(-1)[order]
    counts = [int((deg == d).sum()) for d in range(4)]
    books, geom = np.empty((20, 256), np.float32), []
    opacity = np.clip(g["opacity"][order], 1e-4, 1 - 1e-4)
    for book, x in ((16, np.log(opacity / (1 - opacity))), (17, np.log(g["scales"][order])),
                    (18, g["rotations"][order][:, :1]), (19, g["rotations"][order][:, 1:])):
        books[book], ids = quantise(x)
        geom.append(ids.reshape(len(order), -1))
    sh = g["sh"][order]   # [P,16,3]
    sh_ids = np.empty(sh.shape, np.uint8)
    for k in range(16):
        books[k], sh_ids[:, k, :] = quantise(sh[:, k, :])
    rows, first = [], 0
    for d, c in enumerate(counts):
        rows.append(sh_ids[first:first + c, :(d + 1) ** 2].reshape(-1))
        first += c
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    qm = QuantisedModel(dev(g["means3D"][order].astype(np.float16)), dev(np.concatenate(geom, axis=1)), dev(np.concatenate(rows)),
                        dev(books), counts)
    return w, cam, qm, dev(sh_ids.astype(np.int32)), counts


def index_add_formulation(qm, sh_ids, counts):
    """-> body(grads) -> [20,256]: one index_add_ per codebook over the column of its owners (a suffix of the sorted model)."""
    P = qm.P
    starts = [0] + [counts[0]] * 3 + [counts[0] + counts[1]] * 5 + [P - counts[3]] * 7   # coefficient k: degrees with (d+1)^2 > k
    idx = [sh_ids[starts[k]:, k, :].reshape(-1).contiguous() for k in range(16)]
    geom = qm.geom_ids.to(torch.int32)
    gidx = [geom[:, 0].contiguous(), geom[:, 1:4].reshape(-1).contiguous(), geom[:, 4].contiguous(),
            geom[:, 5:8].reshape(-1).contiguous()]

    def body(dc, rest, opacity, scaling, rotation):
        out = torch.zeros((20, 256), device=dc.device)
        out[0].index_add_(0, idx[0], dc.reshape(-1))
        for k in range(1, 16):
            out[k].index_add_(0, idx[k], rest[starts[k]:, k - 1, :].reshape(-1))
        out[16].index_add_(0, gidx[0], opacity.reshape(-1))
        out[17].index_add_(0, gidx[1], scaling.reshape(-1))
        out[18].index_add_(0, gidx[2], rotation[:, 0])
        out[19].index_add_(0, gidx[3], rotation[:, 1:].reshape(-1))
        return out
    return body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", nargs="*", default=list(DEFAULT))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantised_finetune_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quantised_finetune_bench.py needs a GPU")
    pipe = argparse.Namespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    for name in args.workloads:
        w, cam, qm, sh_ids, counts = quantised_workload(name)
        P = qm.P
        gen = torch.Generator(device="cuda").manual_seed(0)
        grads = [torch.randn(s, device="cuda", generator=gen) for s in ((P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4))]
        ids = (qm.geom_ids, qm.sh_ids, qm.per_band, qm.cumsum, qm.coeffs)
        torch_body = index_add_formulation(qm, sh_ids, counts)
        legs = {"kernel": lambda: _C.quantised_codebook_grad(*ids, *grads), "index_add": lambda: torch_body(*grads)}
        a, b = legs["kernel"](), legs["index_add"]()
        agree = float((a - b).abs().max() / b.abs().max())
        for body in legs.values():
            timed(body, 3)
        blocks = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, body in legs.items():
                blocks[k].append(timed(body, args.iters))
        del grads, sh_ids, torch_body, legs, a, b
        torch.cuda.empty_cache()
        # a whole fine-tune step
        view = argparse.Namespace(image_height=cam.image_height, image_width=cam.image_width, FoVx=cam.FoVx, FoVy=cam.FoVy,
                                  **{k: torch.from_numpy(np.ascontiguousarray(getattr(cam, k))).cuda()
                                     for k in ("world_view_transform", "full_proj_transform", "camera_center")})
        bg = torch.zeros(3, device="cuda")
        with torch.no_grad():
            target = render(view, qm, pipe, bg)["render"].clone()
            target = (target + 0.05 * torch.randn(target.shape, device="cuda", generator=gen)).contiguous()
        qm.requires_grad_(codebooks=True, xyz=True)
        opt = r3dgs_optim.Adam(qm.parameters(), lr=1e-4, eps=1e-15)

        def step():
            opt.zero_grad(set_to_none=True)
            l1_loss(render(view, qm, pipe, bg)["render"], target).backward()
            opt.step()
        timed(step, 3)
        blocks["step"] = [timed(step, args.iters) for _ in range(args.rounds)]
        med = {k: float(np.median(v)) for k, v in blocks.items()}
        nbytes = P * (236 + 8) + int(qm.sh_ids.numel())
        out = {"tool": "quantised_finetune_bench", "workload": name, "P": P, "per_degree": counts, "image": [w["W"], w["H"]],
               "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "call_ms": med,
               "blocks_ms": blocks, "kernel_bytes": nbytes, "kernel_TBps": nbytes / (med["kernel"] * 1e-3) / 1e12,
               "workspace_bytes": int(_C._lib.r3dgs_quantised_codebook_grad_workspace_bytes(P)),
               "index_add_over_kernel": med["index_add"] / med["kernel"], "max_rel_diff_kernel_vs_index_add": agree}
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del qm, opt, target
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
