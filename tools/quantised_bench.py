"""The inference forward over the quantised model against the fp32 ragged inference forward of the same model.

    python tools/quantised_bench.py [--workload metric_500k_1600x1062 garden_like_2M_1600x1062 train_like_6M_1920x1080]
                                    [--rounds 3] [--steps 50] [--out profiles/quantised_bench.jsonl] [--no-trace]

Forward only, one GPU visit.  Per workload:
  prepare   synth_scene's Gaussians with a mixed-degree assignment, sorted by degree; twenty 256-entry codebooks built from
            the scene's own values by kmeans_cuda (as produce_clusters does); ids, half positions and codebooks saved once;
  fp32      rasterize_gaussians_variableSH_bands over the DECODED model (dense decode -> activate_params -> the ragged fp32
            SH buffer): what load_ply + render cost before;
  quant     rasterize_gaussians_quantised over the ids in place.
The two forms alternate `--rounds` times; each timed block is a process of its own under `timeout -k 10`, and the chain ends
at the first failure.  Then one `rocprofv3 --kernel-trace --stats` run per form gives the per-stage kernel times.  One JSON
line per workload: ms per frame of both forms (median, every block, the fp32 blocks' min-to-max spread), kernel times of
the per-Gaussian stages, resident bytes of both models, and whether the quantised form held the bar (median <= the fp32
median + that spread)."""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "reduced-3dgs_amd")]
SCRATCH = os.path.join(os.environ.get("R3DGS_OUT", os.path.join(ROOT, "out")), "quantised_bench")
DEFAULT = ["metric_500k_1600x1062", "garden_like_2M_1600x1062", "train_like_6M_1920x1080"]
STAGES = {"geometry": ("preprocess_geom_kernel",), "depth sort + colour": ("depth_sort_color", "depth_colscan_kernel"),
          "binning": ("emit_pairs_kernel", "radix_", "tile_ranges_kernel"), "blend": ("blend_fwd_kernel",)}


def prepare(wl):
    """-> out/quantised_bench/<wl>.pt: the quantised model of the workload's scene (host tensors)."""
    import numpy as np
    import torch

    import synth_scene as ss
    from diff_gaussian_rasterization import _C
    w = ss.WORKLOADS[wl]
    cam = ss.make_camera(w["W"], w["H"], w["f"], None)
    g = ss.make_gaussians(w["P"], cam, seed=0, degree_mode="mixed", scale_mu=w.get("scale_mu", 0.012))
    order = np.argsort(g["degrees"].reshape(-1), kind="stable")
    g = {k: v[order] for k, v in g.items()}
    counts = [int((g["degrees"] == d).sum()) for d in range(4)]
    P = w["P"]
    dev = torch.device("cuda", 0)

    def book(values):   # values [P', cols] -> (uint8 ids, 256 half-rounded centres), Lloyd from evenly spaced centres
        v = torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev).reshape(-1, 1)
        lo, hi = float(v.min()), float(v.max())
        ids, centres = _C.kmeans_cuda(v, torch.linspace(lo, hi, 256, device=dev), 1e-4, 30)
        return ids.reshape(values.shape).to(torch.uint8).cpu(), centres.half().float().cpu()
    first = np.concatenate([[0], np.cumsum(counts)])
    books, sh_cols = [], []
    for k in range(16):   # coefficient k is stored by the Gaussians of degree >= ceil(sqrt(k + 1)) - 1
        dmin = int(np.ceil(np.sqrt(k + 1))) - 1
        ids, c = book(g["sh"][first[dmin]:, k, :])
        books.append(c)
        sh_cols.append((dmin, ids))
    sh = []
    for d in range(4):
        rows = [ids[first[d] - first[dmin]:first[d + 1] - first[dmin]] for dmin, ids in sh_cols[:(d + 1) ** 2]]
        sh.append(torch.stack(rows, dim=1).reshape(-1))   # [n, K, 3]
    geom = []
    for values in (g["opacity"], np.log(g["scales"]), g["rotations"][:, :1], g["rotations"][:, 1:]):
        ids, c = book(values)
        books.append(c)
        geom.append(ids)
    os.makedirs(SCRATCH, exist_ok=True)
    torch.save(dict(xyz=torch.from_numpy(g["means3D"]).half(), geom_ids=torch.cat(geom, dim=1), sh_ids=torch.cat(sh),
                    codebooks=torch.stack(books), counts=counts, P=P), os.path.join(SCRATCH, wl + ".pt"))


def worker(form, wl, steps, warmup):
    """One timed block of one form -> a JSON line."""
    import numpy as np
    import torch

    import synth_scene as ss
    from diff_gaussian_rasterization import _C
    from r3dgs_quantised import QuantisedModel
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    w = ss.WORKLOADS[wl]
    cam = ss.make_camera(w["W"], w["H"], w["f"], None)
    m = torch.load(os.path.join(SCRATCH, wl + ".pt"))
    qm = QuantisedModel(m["xyz"].to(dev), m["geom_ids"].to(dev), m["sh_ids"].to(dev), m["codebooks"].to(dev), m["counts"])
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    bg, vm, pm, cp = dv(np.zeros(3, np.float32)), dv(cam.world_view_transform), dv(cam.full_proj_transform), dv(cam.camera_center)
    H, W = w["H"], w["W"]
    if form == "quant":
        resident = qm.nbytes

        def frame():
            return _C.rasterize_gaussians_quantised(bg, qm.xyz, qm.geom_ids, qm.sh_ids, qm.codebooks, 1.0, vm, pm, cam.tanfovx,
                                                    cam.tanfovy, H, W, qm.per_band, qm.cumsum, qm.coeffs, cp, False, False)
    else:
        d = qm.decode()
        scales, rotations = _C.activate_params(d["_scaling"], d["_rotation"])
        full = torch.cat((d["_features_dc"], d["_features_rest"]), dim=1)
        rows, first = [], 0
        for deg, n in enumerate(qm.per_band_count):
            rows.append(full[first:first + n, :(deg + 1) ** 2].reshape(-1))
            first += n
        sh, xyz, opacity, degrees = torch.cat(rows).contiguous(), d["_xyz"], d["_opacity"], d["_degrees"]
        # what load_ply keeps resident (dense, every row padded to degree 3) -- the ragged buffer is built from it per frame
        # by the reference's render; here it is built once and only the forward is timed
        resident = sum(t.numel() * t.element_size() for t in d.values())
        ragged = sum(t.numel() * t.element_size() for t in (xyz, opacity, scales, rotations, sh, degrees))
        del d, full, rows, qm
        empty = torch.Tensor([])
        tables = (torch.tensor([1, 4, 9, 16], dtype=torch.int32, device=dev), torch.tensor(m["counts"], dtype=torch.int32, device=dev))
        cumsum = torch.cumsum(tables[1], 0).to(torch.int32)

        def frame():
            return _C.rasterize_gaussians_variableSH_bands(bg, xyz, empty, opacity, scales, rotations, 1.0, empty, vm, pm,
                                                           cam.tanfovx, cam.tanfovy, H, W, sh, tables[1], cumsum, tables[0],
                                                           degrees, cp, False, False)
    torch.cuda.empty_cache()
    with torch.no_grad():
        for _ in range(warmup):
            out = frame()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = frame()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
    res = dict(form=form, workload=wl, ms_per_frame=ms, steps=steps, num_rendered=int(out[0]), resident_bytes=int(resident),
               image_sum=float(out[1].double().sum()), passes=_C.pass_stats())
    if form == "fp32":
        res["ragged_input_bytes"] = int(ragged)
    print(json.dumps(res), flush=True)


def run(cmd, limit, log):
    """One child under `timeout -k 10`; -> its last JSON line, or None when it failed (the caller ends the chain)."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, cwd=ROOT)
    log.write(f"$ {' '.join(cmd)}\nrc={r.returncode}\n{r.stdout[-4000:]}{r.stderr[-4000:]}\n")
    log.flush()
    if r.returncode != 0:
        print(f"FAILED (rc={r.returncode}): {' '.join(cmd)}\n{r.stderr[-2000:]}", flush=True)
        return None
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else {}


def stage_times(csv_path, frames):
    """us per frame of each forward stage from a rocprofv3 kernel-stats table."""
    us = {k: 0.0 for k in STAGES}
    kernels = {}
    for r in csv.DictReader(open(csv_path)):
        name = r["Name"].split("(")[0].replace("void ", "").replace("r3::", "")
        for stage, keys in STAGES.items():
            if any(k in name for k in keys):
                us[stage] += float(r["TotalDurationNs"]) / 1e3 / frames
                kernels[name] = round(float(r["TotalDurationNs"]) / 1e3 / frames, 2)
    return {k: round(v, 2) for k, v in us.items()}, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms (at least three)")
    ap.add_argument("--steps", type=int, default=50, help="frames per timed block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantised_bench.jsonl"))
    ap.add_argument("--no-trace", action="store_true", help="skip the two rocprofv3 runs")
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process, seconds")
    ap.add_argument("--prepare", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", choices=["fp32", "quant"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.prepare:
        return prepare(args.prepare)
    if args.worker:
        return worker(args.worker, args.workload[0], args.steps, args.warmup)
    import numpy as np
    me = [sys.executable, os.path.abspath(__file__)]
    os.makedirs(SCRATCH, exist_ok=True)
    log = open(os.path.join(SCRATCH, "children.log"), "a")
    for wl in args.workload:
        if run(me + ["--prepare", wl], 2 * args.limit, log) is None:   # scene generation and twenty k-means
            return 1
        blocks = {"fp32": [], "quant": []}
        for _ in range(max(args.rounds, 3)):
            for form in ("fp32", "quant"):
                r = run(me + ["--worker", form, "--workload", wl, "--steps", str(args.steps), "--warmup", str(args.warmup)],
                        args.limit, log)
                if r is None:
                    return 1
                blocks[form].append(r)
        ms = {f: [b["ms_per_frame"] for b in blocks[f]] for f in blocks}
        spread = max(ms["fp32"]) - min(ms["fp32"])
        out = dict(metric="quantised_forward", workload=wl, gaussians=None, per_degree=None, frames_per_block=args.steps,
                   ms_per_frame={f: float(np.median(v)) for f, v in ms.items()}, ms_all=ms, fp32_spread_ms=spread,
                   holds_bar=bool(np.median(ms["quant"]) <= np.median(ms["fp32"]) + spread),
                   resident_bytes={"fp32_dense": blocks["fp32"][0]["resident_bytes"], "quantised": blocks["quant"][0]["resident_bytes"],
                                   "fp32_ragged_inputs": blocks["fp32"][0]["ragged_input_bytes"]},
                   same_image=blocks["fp32"][0]["image_sum"] == blocks["quant"][0]["image_sum"],
                   num_rendered=blocks["quant"][0]["num_rendered"], passes=blocks["quant"][-1]["passes"])
        import torch
        m = torch.load(os.path.join(SCRATCH, wl + ".pt"))
        out["gaussians"], out["per_degree"] = m["P"], m["counts"]
        del m
        if not args.no_trace:
            frames = 10
            out["stage_us"], out["kernel_us"] = {}, {}
            for form in ("fp32", "quant"):
                d = os.path.join(SCRATCH, f"trace_{wl}_{form}")
                shutil.rmtree(d, ignore_errors=True)
                # every frame of the traced child counts: warm-up 0, and the decode / activate kernels are not forward stages
                r = run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--"] + me +
                        ["--worker", form, "--workload", wl, "--steps", str(frames), "--warmup", "0"], args.limit, log)
                if r is None:
                    return 1
                found = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
                if found:
                    out["stage_us"][form], out["kernel_us"][form] = stage_times(found[0], frames)
        print(json.dumps(out), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(out) + "\n")
        os.remove(os.path.join(SCRATCH, wl + ".pt"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
