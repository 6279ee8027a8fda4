"""Static listing of the two blend kernels' inner loops, from the gfx950 assembly of this tree's build (no GPU needed):
    python tools/blend_isa.py [--label TEXT] [--src DIR] [-D...] >> profiles/blend_inner_loop_isa.txt
Compiles csrc/blend.hip (of this tree, or of another checkout's csrc with --src) with the flags of reduced-3dgs_amd/build.py and
prints, for blend_fwd_kernel<1, false> and blend_bwd_kernel<4, true, false>, the instructions of three regions
  * trip:      the entry loop body (forward: the batch-of-four loop, i.e. four trips; backward: one entry = four quadrant trips
               and the per-entry shared part), without the reduction blocks;
  * reduce:    the per-entry reduction of the backward (DPP adds, cross-row exchange, LDS store, clearing the nine sums);
  * preamble:  what a 64-entry chunk pays once (staging, region pre-test or mask fetch, prefetch, and the backward's flush),
grouped by the counter classes of bench.py VALU_CYCLES and priced with them; an ADD / MUL / FMA / TRANS instruction with an
SGPR source or a DPP control is priced at the slow rate (4.1, profiles/r03_valu_rate.txt) and listed.  Also listed: every
v_cmp feeding a v_cndmask, every v_mov, every v_readlane / v_readfirstlane, and the SALU, LDS and branch counts.  The regions
are found from the compiler's own loop annotations; the labels of the blocks taken are printed so that they can be checked
against the assembly (kept with --keep-asm FILE)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reduced-3dgs_amd"))
sys.path.insert(0, ROOT)
import build as b  # noqa: E402

RATES = {"ADD_F32": 2.4, "MUL_F32": 2.4, "FMA_F32": 2.6, "TRANS_F32": 8.1, "INT32": 4.1, "CVT": 4.1, "other": 4.1}
try:   # bench.py is the yardstick; the table above is only the fallback when it cannot be imported (torch missing)
    from bench import VALU_CYCLES  # noqa: E402
    RATES = {k.replace("SQ_INSTS_VALU_", ""): v for k, v in VALU_CYCLES.items()}
except Exception:  # pragma: no cover
    pass
SLOW = RATES["other"]
KERNELS = {"blend_fwd_kernel<1, false>": "blend_fwd_kernelILi1ELb0E", "blend_bwd_kernel<4, true, false>": "blend_bwd_kernelILi4ELb1ELb0E"}
INT_OPS = re.compile(r"v_(add|sub|subrev|addc|subb|add3|lshl_add|lshl_or|and_or|or3|xad|mad|mul_lo|mul_hi|mul|and|or|xor|not|lshl|lshr|ashr|"
                     r"lshlrev|lshrrev|ashrrev|bfe|bfi|min|max|med3|min3|max3|mbcnt|bcnt|ffbh|ffbl|cmp_\w+|cmpx_\w+|alignbit|perm)"
                     r"(_co|_lo|_hi)?_[iu](16|24|32|64)")


def classify(op):
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
    if re.match(r"v_(add|sub|subrev)_f32$", base):
        return "ADD_F32"
    if re.match(r"v_mul(_legacy)?_f32$", base):
        return "MUL_F32"
    if re.match(r"v_(fma|fmac|mad|mac)_f32$", base):
        return "FMA_F32"
    if re.match(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)(_legacy|_iflag)?_f32$", base):
        return "TRANS_F32"
    if base.startswith("v_cvt_"):
        return "CVT"
    if INT_OPS.match(base) or re.match(r"v_(mad_u64_u32|mad_i64_i32|lshl_add_u64|mul_u32_u24|mad_u32_u24|add_u32|sub_u32)", base):
        return "INT32"
    return "other"


def sgpr_source(op, args):
    """True if a SOURCE operand is an SGPR (not the vcc / sgpr-pair destination of a compare, not a select's mask)."""
    ops = [a.strip() for a in args.split(",")]
    srcs = ops[1:]
    if op.startswith(("v_cmp", "v_readlane", "v_readfirstlane")) or "_co_" in op:
        srcs = ops[1:] if op.endswith("_e64") else ops
        if op.endswith("_e32") and op.startswith("v_cmp"):
            srcs = ops[1:]
    if op.startswith("v_cndmask") and op.endswith("_e64"):
        srcs = ops[1:3]
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return False
    return any(re.match(r"^[-|]*s(\d+|\[\d+:\d+\])\|?$", s.split(" ")[0]) for s in srcs)


def parse_blocks(lines):
    """[(label, is_inner_header, loop header this block belongs to (innermost) or None, depth, [instruction lines])]"""
    blocks, cur = [], None
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):|^; (%bb\.\d+):", ln)
        if m:
            cur = dict(label=(m.group(1) or m.group(2)).lstrip("."), inner=False, loop=None, depth=0, parent=None, ins=[])
            blocks.append(cur)
        if cur is None:
            cur = dict(label="entry", inner=False, loop=None, depth=0, parent=None, ins=[])
            blocks.append(cur)
        h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", ln)
        if h:
            cur["loop"], cur["depth"] = "L" + h.group(1), int(h.group(2))
        if re.search(r"=>\s*This (Inner )?Loop Header: Depth=(\d+)", ln):
            cur["loop"], cur["depth"] = cur["label"], int(re.search(r"Depth=(\d+)", ln).group(1))
            cur["inner"] = "Inner Loop Header" in ln
        p = re.search(r"Parent Loop (BB\d+_\d+) Depth=", ln)
        if p:
            cur["parent"] = "L" + p.group(1)
        s = ln.strip()
        if s and not s.startswith((";", ".")) and not re.match(r"^\S+:$", s.split(";")[0].strip()):
            cur["ins"].append(s.split(";")[0].strip())
    return blocks


def summarise(name, blocks, out):
    ins = [i for bl in blocks for i in bl["ins"] if not i.startswith(("s_waitcnt", "s_nop"))]
    valu = [i for i in ins if i.startswith("v_")]
    counts = {k: 0 for k in RATES}
    weighted = weighted_plain = 0.0
    slow_src, movs, lanes, pairs = [], [], [], []
    last_cmp = {}
    for i in valu:
        op, _, args = i.partition(" ")
        c = classify(op)
        counts[c] += 1
        special = sgpr_source(op, args) or "_dpp" in op or "row_" in args or "quad_perm" in args
        rate = max(RATES[c], SLOW) if special and c != "TRANS_F32" else RATES[c]
        weighted += rate
        weighted_plain += RATES[c]
        if special and RATES[c] < SLOW:
            slow_src.append(i)
        if op.startswith("v_mov"):
            movs.append(i)
        if op.startswith(("v_readlane", "v_readfirstlane")):
            lanes.append(i)
        if op.startswith("v_cmp"):
            dst = "vcc" if op.endswith("_e32") else args.split(",")[0].strip()
            last_cmp[dst] = i
        if op.startswith("v_cndmask"):
            mask = "vcc" if op.endswith("_e32") else args.split(",")[-1].strip()
            pairs.append((last_cmp.get(mask, "(mask from outside the region)"), i))
    salu = [i for i in ins if i.startswith("s_") and not i.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier"))]
    slow = counts["INT32"] + counts["CVT"] + counts["other"]
    out.append(f"  [{name}] blocks: {' '.join(bl['label'] for bl in blocks)}")
    out.append("    VALU %d: %s" % (len(valu), "  ".join(f"{k} {v}" for k, v in counts.items())))
    out.append(f"    slow class (INT32 + CVT + other) {slow};  fast-class instructions with an SGPR source or DPP {len(slow_src)}")
    out.append(f"    weighted cycles {weighted:.1f}  (every class at its own rate, ignoring SGPR sources / DPP: {weighted_plain:.1f})")
    out.append("    SALU %d  LDS %d  VMEM %d  branches %d" % (
        len(salu), sum(i.startswith("ds_") for i in ins), sum(i.startswith(("global_", "flat_", "scratch_", "buffer_")) for i in ins),
        sum(i.startswith(("s_cbranch", "s_branch")) for i in ins)))
    if any(i.startswith("scratch_") for i in ins):
        out.append("    SCRATCH ACCESS IN THIS REGION: " + "; ".join(i for i in ins if i.startswith("scratch_")))
    for title, lst in (("SGPR-source / DPP in a fast class", slow_src), ("v_mov", movs), ("readlane", lanes)):
        if lst:
            out.append(f"    {title} ({len(lst)}):")
            out.extend("        " + i for i in lst)
    if pairs:
        out.append(f"    v_cmp -> v_cndmask pairs ({len(pairs)}):")
        out.extend(f"        {c}  ->  {s}" for c, s in pairs)
    return dict(valu=len(valu), slow=slow, weighted=weighted, plain=weighted_plain, salu=len(salu), counts=counts)


def regions(blocks):
    n_exp = {}
    for bl in blocks:
        if bl["loop"]:
            n_exp[bl["loop"]] = n_exp.get(bl["loop"], 0) + sum(i.startswith("v_exp_f32") for i in bl["ins"])
    inner = {bl["label"] for bl in blocks if bl["inner"]}
    trip_loop = max((k for k in n_exp if k in inner), key=lambda k: n_exp[k])
    body = [bl for bl in blocks if bl["loop"] == trip_loop]
    def is_reduce(bl):
        t = bl["ins"]
        zero_movs = sum(bool(re.match(r"v_mov_b32_e32 v\d+, 0$", i)) for i in t)
        valu = sum(i.startswith("v_") for i in t)
        return (any("row_ror" in i or "ds_bpermute" in i for i in t) or zero_movs >= 3 or
                (valu <= 2 and any(i.startswith("ds_write_b32") for i in t)) or
                (valu == 0 and sum(i.startswith("ds_read") for i in t) >= 3))
    reduce_ = [bl for bl in body if is_reduce(bl)]
    trip = [bl for bl in body if not is_reduce(bl)]
    head = next(bl for bl in blocks if bl["label"] == trip_loop)
    if head["parent"]:
        pre = [bl for bl in blocks if bl["loop"] == head["parent"]]
    else:   # the chunk loop is not a natural loop in this build: from the staging stores to the first inner loop, in text order
        start = next(k for k, bl in enumerate(blocks) if any(i.startswith("ds_write_b64") for i in bl["ins"]))
        pre = []
        for bl in blocks[start:]:
            if bl["inner"]:
                break
            if bl["loop"] not in inner:
                pre.append(bl)
    return trip_loop, n_exp[trip_loop], trip, reduce_, pre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--src", default=b.CSRC, help="csrc directory to compile (another checkout's, for the parent's listing)")
    ap.add_argument("--keep-asm", default=None)
    ap.add_argument("-D", action="append", default=[], dest="defs")
    a = ap.parse_args()
    flags = [a.src if f == b.CSRC else f for f in b.COMMON + b.UNITS["blend.hip"] if f != "-fPIC"] + ["-D" + d for d in a.defs]
    with tempfile.TemporaryDirectory() as tmp:
        asm = a.keep_asm or os.path.join(tmp, "blend.s")
        subprocess.run([b.HIPCC] + flags + ["--cuda-device-only", "-S", "-o", asm, os.path.join(a.src, "blend.hip")],
                       check=True, stderr=subprocess.DEVNULL)
        txt = open(asm).read()
    out = [f"==== {a.label}" + (f"  (-D{' -D'.join(a.defs)})" if a.defs else ""),
           "rates (cycles per wave64 instruction per SIMD): " + "  ".join(f"{k} {v}" for k, v in RATES.items())]
    res = {}
    for pretty, mangled in KERNELS.items():
        sym = re.search(r"^(_ZN2r3\d+" + re.escape(mangled) + r"\w*):", txt, re.M).group(1)
        body = txt[txt.index("\n" + sym + ":"):]
        body = body[:body.index(".Lfunc_end")]
        meta = txt[txt.index(".amdgpu_metadata"):]
        blk = meta[meta.index(".name:           " + sym) - 1200:meta.index(".name:           " + sym) + 600]
        get = lambda k, s=blk: int(re.findall(r"\." + k + r":\s+(\d+)", s)[-1 if k in ("agpr_count",) else 0])  # noqa: E731
        m2 = meta[meta.index(".name:           " + sym):]
        vg, sg_, scr = (int(re.search(r"\." + k + r":\s+(\d+)", m2).group(1)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size"))
        blocks = parse_blocks(body.splitlines())
        loop, nexp, trip, red, pre = regions(blocks)
        out.append(f"\n== {pretty}: VGPR {vg}  SGPR {sg_}  scratch {scr} B  waves/SIMD {min(8, 512 // ((vg + 7) // 8 * 8))};"
                   f"  trip loop {loop} holds {nexp} v_exp_f32 = {nexp} (entry, quadrant) trips per pass of its body")
        r = {"trip": summarise("trip x%d" % nexp, trip, out)}
        if red:
            r["reduce"] = summarise("reduce (per entry with a hit)", red, out)
        r["preamble"] = summarise("preamble (per 64-entry chunk)", pre, out)
        t = r["trip"]
        out.append(f"  per (entry, quadrant) trip, every branch taken: VALU {t['valu'] / nexp:.2f}  slow class {t['slow'] / nexp:.2f}  "
                   f"weighted cycles {t['weighted'] / nexp:.1f}  SALU {t['salu'] / nexp:.2f}")
        res[pretty] = (r, nexp)
    print("\n".join(out))
    return res


if __name__ == "__main__":
    main()
