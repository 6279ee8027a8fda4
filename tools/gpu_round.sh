#!/bin/bash
# One GPU-box visit: smoke, -m gpu parity tests, bench, rocprofv3 kernel stats (+ optional PMC pass and
# tuning-knob sweeps).  Every command is wrapped in its own `timeout` so a hang cannot eat the round's GPU
# budget.  Outputs land in $OUT/ (copy what should be judged into profiles/).
set -u
# logs, traces and summaries of this script: $R3DGS_OUT, relative to the repository root (the working directory) or
# absolute, default out/; made absolute here so that steps run from another directory and the Python tools agree
OUT=${R3DGS_OUT:-out}; case $OUT in /*) ;; *) OUT=$PWD/$OUT ;; esac; export R3DGS_OUT=$OUT
mkdir -p $OUT
export PYTHONPATH=$PWD:$PWD/reduced-3dgs_amd
export TMPDIR=/tmp
ROOT=$PWD
S=$OUT/summary.log; : > $S
if [ "${SMOKE:-1}" = "1" ]; then
  ( timeout ${T_SMOKE:-300} python -c "import __graft_entry__ as g; g.smoke()" ) > $OUT/smoke.log 2>&1; echo "smoke rc=$?" >> $S
fi
if [ "${TESTS:-1}" = "1" ]; then
  ( timeout ${T_TEST:-420} python -m pytest ${PYTEST_TARGET:-tests} -m gpu -x -q ${PYTEST_ARGS:-} ) > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $S
fi
if [ "${BENCH:-1}" = "1" ]; then
  ( timeout ${T_BENCH:-240} python bench.py --full --steps ${STEPS:-20} --warmup 5 ) > $OUT/bench.log 2>&1; echo "bench rc=$?" >> $S
fi
if [ -n "${EXTRA:-}" ]; then   # one extra in-repo python script (e.g. tools/reduction_bench.py)
  ( timeout ${T_EXTRA:-240} python $EXTRA ) > $OUT/extra.log 2>&1; echo "extra rc=$?" >> $S
fi
# tuning sweeps: "NAME=VALUE NAME=VALUE;NAME=VALUE" -> one short bench per ';'-separated env set
if [ -n "${SWEEP:-}" ]; then
  IFS=';' read -ra SETS <<< "$SWEEP"
  for envset in "${SETS[@]}"; do
    tag=$(echo "$envset" | tr ' =' '__')
    ( env $envset timeout ${T_BENCH:-240} python bench.py --full --steps ${STEPS:-20} --warmup 5 --no-cpu-baseline ) > $OUT/bench_$tag.log 2>&1
    echo "sweep [$envset] rc=$? $(tail -1 $OUT/bench_$tag.log | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(d["value"], {k:v["avg_ms"] for k,v in d["stages"].items()}, d["render_fps"])' 2>/dev/null)" >> $S
  done
fi
if [ "${PROF:-1}" = "1" ]; then
  ( cd /tmp && timeout ${T_PROF:-240} rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r -- python $ROOT/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline ) > $OUT/prof.log 2>&1; echo "prof rc=$?" >> $S
fi
if [ -n "${EXTRA_PROF:-}" ]; then   # kernel stats of an extra in-repo script
  ( cd /tmp && timeout ${T_PROF:-240} rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_extra -o r -- python $ROOT/$EXTRA_PROF ) > $OUT/prof_extra.log 2>&1; echo "prof_extra rc=$?" >> $S
  f=$(find $OUT/prof_extra -name "*kernel_stats.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $OUT/extra_kernel_stats.csv
fi
if [ "${LISTCTR:-0}" = "1" ]; then ( cd /tmp && timeout 60 rocprofv3 -L ) > $OUT/counters.txt 2>&1; fi
if [ -n "${PMC:-}" ]; then   # separate counter passes, kernel-trace only (never mixed with sys/hip traces)
  i=0
  IFS=';' read -ra PASSES <<< "$PMC"
  for ctrs in "${PASSES[@]}"; do
    ( cd /tmp && timeout ${T_PROF:-240} rocprofv3 --kernel-trace --pmc $ctrs --output-format csv -d $OUT/pmc$i -o r -- python $ROOT/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline ) > $OUT/pmc$i.log 2>&1; echo "pmc$i [$ctrs] rc=$?" >> $S
    i=$((i+1))
  done
fi
cat $S; echo ---; tail -5 $OUT/smoke.log 2>/dev/null; echo ---; tail -30 $OUT/pytest_gpu.log 2>/dev/null; echo ---; tail -1 $OUT/bench.log 2>/dev/null; echo ---; tail -${EXTRA_TAIL:-30} $OUT/extra.log 2>/dev/null
f=$(find $OUT/prof -name "*kernel_stats.csv" 2>/dev/null | head -1); if [ -n "$f" ]; then echo "--- $f"; head -22 "$f" | cut -c1-200; fi
if [ -f $OUT/extra_kernel_stats.csv ] && [ -n "${EXTRA_PROF:-}" ]; then echo "--- extra kernel stats"; head -${EXTRA_STATS_LINES:-25} $OUT/extra_kernel_stats.csv | cut -c1-220; fi
exit 0
