#!/bin/bash
# MFMA-busy share per kernel family over a short bench.py --full run (one PMC pass, no trace
# domains): SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs).
# -> $OUT_DIR/mfma_busy.txt (OUT_DIR defaults to <repo>/bench_out)
R=$(cd "$(dirname "$0")/.." && pwd); OUT_DIR=${OUT_DIR:-$R/bench_out}
OUT=$OUT_DIR/mfma_pmc; rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_MFMA --output-format csv -d $OUT -o p -- \
  python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-nocfg --attn-reps 3 ${BENCH_ARGS:-} > $OUT/run.log 2>&1 || { tail -5 $OUT/run.log; exit 1; }
python3 $R/tools/mfma_busy.py $OUT $OUT_DIR/${ROUND:-r01}_mfma_busy.json > $OUT_DIR/mfma_busy.txt && cat $OUT_DIR/mfma_busy.txt
