"""Memory accesses and waits of the kernels of csrc/preprocess_bwd.hip, counted in the compiler's gfx950 listing (no GPU needed):
    python tools/prebwd_listing.py [--keep DIR] > out/prebwd_listing.txt
Compiles the translation unit with the flags of reduced-3dgs_amd/build.py and prints, per kernel: FLAT and GLOBAL loads / stores,
LDS instructions, s_waitcnt instructions, how many of those are full drains (vmcnt(0) and lgkmcnt(0) in one wait: what a FLAT
access forces, since it counts on both counters), VGPRs and scratch bytes.  --keep DIR leaves the listing there."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reduced-3dgs_amd"))
import build as b  # noqa: E402

UNIT = "preprocess_bwd.hip"


def listing(path):
    flags = [f for f in b.COMMON + b.UNITS[UNIT] if f != "-fPIC"] + os.environ.get("R3DGS_EXTRA_FLAGS", "").split()
    subprocess.run([b.HIPCC] + flags + ["--cuda-device-only", "-S", "-o", path, os.path.join(b.CSRC, UNIT)], check=True,
                   stderr=subprocess.DEVNULL)
    return open(path).read()


def kernels(txt):
    """{mangled name: body} of every function of the listing (label ... .Lfunc_end)"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def count(body):
    ins = [l.split(";")[0].strip() for l in body.splitlines()]
    ins = [l for l in ins if l and not l.startswith((".", "_Z")) and not l.endswith(":")]
    n = lambda p: sum(1 for l in ins if re.match(p, l))  # noqa: E731
    waits = [l for l in ins if l.startswith("s_waitcnt")]
    return dict(flat_ld=n(r"flat_load"), flat_st=n(r"flat_store"), glob_ld=n(r"global_load"), glob_st=n(r"global_store"),
                scalar_ld=n(r"s_load|s_buffer_load"), lds=n(r"ds_"), waits=len(waits),
                drains=sum(1 for l in waits if "vmcnt(0)" in l and "lgkmcnt(0)" in l),
                vm_only=sum(1 for l in waits if "vmcnt" in l and "lgkmcnt" not in l),
                lgkm_only=sum(1 for l in waits if "lgkmcnt" in l and "vmcnt" not in l))


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp:
        if keep:
            os.makedirs(keep, exist_ok=True)
        txt = listing(os.path.join(keep or tmp, UNIT.replace(".hip", ".s")))
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", txt[txt.index(".amdgpu_metadata"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                      int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    ks = kernels(txt)
    names = [k for k in ks if k in meta]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    print(f"{'kernel':44s} {'flat ld':>7s} {'flat st':>7s} {'glob ld':>7s} {'glob st':>7s} {'s_load':>6s} {'ds_*':>5s} {'waits':>5s} "
          f"{'full drains':>11s} {'vmcnt only':>10s} {'lgkm only':>9s} {'VGPR':>5s} {'scratch B':>9s}")
    for k, d in sorted(zip(names, dem), key=lambda t: t[1]):
        c, (vgpr, scratch) = count(ks[k]), meta[k]
        d = re.sub(r"\(.*", "", d.replace("void ", "").replace("r3::", ""))
        print(f"{d:44s} {c['flat_ld']:7d} {c['flat_st']:7d} {c['glob_ld']:7d} {c['glob_st']:7d} {c['scalar_ld']:6d} {c['lds']:5d} "
              f"{c['waits']:5d} {c['drains']:11d} {c['vm_only']:10d} {c['lgkm_only']:9d} {vgpr:5d} {scratch:9d}")


if __name__ == "__main__":
    main()
