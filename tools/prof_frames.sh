#!/bin/bash
# rocprofv3 kernel trace of bench.py --full at each frame count in $FRAMES (default "16 2"),
# summarised per step by tools/prof_summary.py into $OUT_DIR/breakdown_f<F>.txt
# (OUT_DIR defaults to <repo>/bench_out)
export HSA_ENABLE_IPC_MODE_LEGACY=0
R=$(cd "$(dirname "$0")/.." && pwd); OUT_DIR=${OUT_DIR:-$R/bench_out}; mkdir -p $OUT_DIR
cd /tmp && export TMPDIR=/tmp
for f in ${FRAMES:-16 2}; do
  # the raw traces are large: they stay under /tmp, only the summaries go to $OUT_DIR
  RAW=/tmp/vd_prof_f$f; rm -rf $RAW
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $RAW -o run -- python3 $R/bench.py --full --frames $f --steps 6 --warmup 2 --no-cpu-baseline --no-nocfg --attn-reps ${ATTN_REPS:-2} > $OUT_DIR/prof_f$f.log 2>&1 || exit 1
  python3 $R/tools/prof_summary.py $(find $RAW -name "*kernel_trace.csv" | head -1) > $OUT_DIR/breakdown_f$f.txt || exit 1
  cp $(find $RAW -name "*kernel_stats.csv" | head -1) $OUT_DIR/kernel_stats_f$f.csv
  head -3 $OUT_DIR/breakdown_f$f.txt
done
