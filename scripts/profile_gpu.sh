#!/bin/bash
# Runs on the GPU box (via gpurun): rocprofv3 kernel trace + stats, then HBM PMC passes, each in
# its own run (never combined).  Summaries land in gpurun_out/<tag>/; copy what you want judged
# into profiles/.
TAG=${1:-prof}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
ARGS="$R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-extras"
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o bench -- python3 $ARGS > $OUT/trace.log 2>&1
echo "trace rc=$?"
timeout 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o bench -- python3 $ARGS > $OUT/pmc_fetch.log 2>&1
echo "fetch rc=$?"
timeout 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o bench -- python3 $ARGS > $OUT/pmc_write.log 2>&1
echo "write rc=$?"
timeout 300 rocprofv3 --pmc SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --output-format csv -d $OUT/pmc_sq -o bench -- python3 $ARGS > $OUT/pmc_sq.log 2>&1
echo "sq rc=$?"
find $OUT -name "*.csv" | head -20
# keep the merged payload small: drop the per-dispatch kernel trace, keep stats + counters
find $OUT -name "*kernel_trace.csv" -size +8M -delete
du -sh $OUT
