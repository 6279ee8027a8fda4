#!/bin/bash
# One GPU visit: smoke, the driver-form bench line, this tree's library against libr3dgs_hip_old.so (the previous round's
# tree built with R3DGS_BUILD_TAG=old) alternating on the workloads named in $WLS, a kernel trace, then the GPU tests.
set -u
# logs, traces and summaries of this script: $R3DGS_OUT, relative to the repository root (the working directory) or
# absolute, default out/; made absolute here so that steps run from another directory and the Python tools agree
OUT=${R3DGS_OUT:-out}; case $OUT in /*) ;; *) OUT=$PWD/$OUT ;; esac; export R3DGS_OUT=$OUT
mkdir -p $OUT
export PYTHONPATH=$PWD:$PWD/reduced-3dgs_amd TMPDIR=/tmp
ROOT=$PWD
S=$OUT/summary.log; : > $S
( timeout 300 python -c "import __graft_entry__ as g; g.smoke()" ) > $OUT/smoke.log 2>&1; echo "smoke rc=$? $(tail -1 $OUT/smoke.log | cut -c1-200)" >> $S
( timeout 300 python bench.py --full --steps 20 --warmup 5 ) > $OUT/bench.log 2>&1; echo "bench20 rc=$?" >> $S
: > $OUT/ab_rounds.txt
for wl in ${WLS:-metric_500k_1600x1062}; do
  for lib in ${LIBS:-old new old new}; do
    if [ $lib = new ]; then unset R3DGS_LIB; else export R3DGS_LIB=$lib; fi
    line=$(timeout 300 python bench.py --full --workload $wl --steps 20 --warmup 5 --cameras 4 --no-cpu-baseline 2>/dev/null | tail -1 | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["value"], "it/s", d["ms_per_step"], "ms;", " / ".join("%s %.4f" % (k, v["avg_ms"]) for k, v in d["stages"].items()), "; ref-mode", d.get("value_reference_mode"))')
    echo "$wl [$lib] $line" >> $OUT/ab_rounds.txt
  done
done
unset R3DGS_LIB
cat $OUT/ab_rounds.txt >> $S
if [ "${PROF:-1}" = "1" ]; then
  ( cd /tmp && timeout 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r -- python $ROOT/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline ) > $OUT/prof.log 2>&1; echo "prof rc=$?" >> $S
  f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp "$f" $OUT/kernel_stats_metric.csv
fi
if [ "${TESTS:-1}" = "1" ]; then
  ( timeout ${T_TEST:-1200} python -m pytest tests -m gpu -q -s ${PYTEST_ARGS:-} ) > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$? $(tail -1 $OUT/pytest_gpu.log)" >> $S
fi
cat $S
tail -1 $OUT/bench.log | cut -c1-3000
[ -f $OUT/kernel_stats_metric.csv ] && head -24 $OUT/kernel_stats_metric.csv | cut -c1-160
grep -E "FAILED|Error|assert" $OUT/pytest_gpu.log | head -40
exit 0
