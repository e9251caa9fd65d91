#!/bin/bash
# Round checkpoint: all GPU tests, the default bench line with every side measurement (--full),
# then rocprof step breakdowns at 16 and 2 frames (tools/prof_frames.sh).  Stops at the first
# abnormal exit.  Output under $OUT_DIR (default <repo>/bench_out).
export HSA_ENABLE_IPC_MODE_LEGACY=0
R=$(cd "$(dirname "$0")/.." && pwd); export OUT_DIR=${OUT_DIR:-$R/bench_out}
cd $R && mkdir -p $OUT_DIR
timeout -k 10 600 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread > $OUT_DIR/pytest_gpu.log 2>&1
rc=$?; tail -3 $OUT_DIR/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full > $OUT_DIR/bench_default.json 2> $OUT_DIR/bench_default.log || exit 1
cat $OUT_DIR/bench_default.json
[ -n "$NO_PROF" ] && exit $rc
bash tools/prof_frames.sh || exit 1
exit $rc
