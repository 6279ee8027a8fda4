set -u
export PYTHONPATH=$PWD:$PWD/reduced-3dgs_amd TMPDIR=/tmp
# logs, traces and summaries of this script: $R3DGS_OUT, relative to the repository root (the working directory) or
# absolute, default out/; made absolute here so that steps run from another directory and the Python tools agree
OUT=${R3DGS_OUT:-out}; case $OUT in /*) ;; *) OUT=$PWD/$OUT ;; esac; export R3DGS_OUT=$OUT
mkdir -p $OUT
( timeout 240 python bench.py --full --steps 20 --warmup 5 ) > $OUT/bench.log 2>&1; echo "bench20 rc=$?"
( timeout 240 python bench.py --full ) > $OUT/bench_default.log 2>&1; echo "bench50 rc=$?"
bash tools/other_workloads.sh > $OUT/other.log 2>&1
tail -1 $OUT/bench.log | cut -c1-300
