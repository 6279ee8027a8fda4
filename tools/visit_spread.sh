#!/bin/bash
# the driver-form bench line ten times in one visit: how much a single 20-step run scatters
export PYTHONPATH=$PWD:$PWD/reduced-3dgs_amd TMPDIR=/tmp
# logs, traces and summaries of this script: $R3DGS_OUT, relative to the repository root (the working directory) or
# absolute, default out/; made absolute here so that steps run from another directory and the Python tools agree
OUT=${R3DGS_OUT:-out}; case $OUT in /*) ;; *) OUT=$PWD/$OUT ;; esac; export R3DGS_OUT=$OUT
mkdir -p $OUT
: > $OUT/bench_spread.txt
for i in 1 2 3 4 5 6 7 8 9 10; do
  timeout 200 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"], d["value_reference_mode"], d["value_sh_sparsity"], d["host"]["gpu_event_ms_per_step"])' >> $OUT/bench_spread.txt
done
cat $OUT/bench_spread.txt
