#!/bin/bash
# bench (default args, --full: with the roofline timings and the CPU baseline) + rocprofv3
# kernel-trace/stats of a short bench.  Output under $OUT_DIR (default <repo>/bench_out).
R=$(cd "$(dirname "$0")/.." && pwd); OUT_DIR=${OUT_DIR:-$R/bench_out}
cd $R && mkdir -p $OUT_DIR/prof
export HSA_ENABLE_IPC_MODE_LEGACY=0
if [ -n "$PYTEST_K" ]; then
  if [ "$PYTEST_K" = "all" ]; then KARG=(); else KARG=(-k "$PYTEST_K"); fi
  timeout -k 10 900 python -m pytest tests -m gpu -q -rf "${KARG[@]}" > $OUT_DIR/pytest_gpu.log 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -15 $OUT_DIR/pytest_gpu.log
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
fi
if [ -z "$NO_BENCH" ]; then
  timeout -k 10 900 python bench.py --full $BENCH_ARGS > $OUT_DIR/bench_default.log 2>&1
  rc=$?; echo "bench rc=$rc"; tail -3 $OUT_DIR/bench_default.log
  [ $rc -ne 0 ] && exit $rc
fi
cd /tmp && export TMPDIR=/tmp
# --full: tools/prof_summary.py also reads the roofline launches that follow the step loop
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof -o run -- python3 $R/bench.py --full --steps ${PROF_STEPS:-5} --warmup 2 --no-cpu-baseline --no-nocfg $PROF_ARGS > $OUT_DIR/prof/bench_prof.log 2>&1
rc=$?; echo "rocprof rc=$rc"; tail -2 $OUT_DIR/prof/bench_prof.log
find $OUT_DIR/prof -name "*.csv" | head
exit $rc
