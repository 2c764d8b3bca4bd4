#!/bin/bash
# usage (GPU box): tools/pmc.sh <tag> [bench args]   -- one rocprofv3 --pmc pass per TCC counter group,
# each under its own time limit (MI355X_MICROARCH.md "HBM" / "rocprofv3 PMC slots": FETCH_SIZE and
# WRITE_SIZE cannot share a pass).  Summary -> $OUT/pmc_<tag>.json (tools/pmc_summary.py; OUT defaults to bench_out).
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
TAG=$1; shift
mkdir -p $OUT
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout -s KILL 240 rocprofv3 --pmc $ctr --kernel-trace -d $OUT/pmc_${TAG}_$ctr -o run --output-format csv \
    -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-ingest --c4-strong off "$@" > $OUT/pmc_${TAG}_$ctr.log 2>&1 \
    || { echo "pmc pass $ctr failed"; tail -20 $OUT/pmc_${TAG}_$ctr.log; exit 1; }
done
python3 tools/pmc_summary.py $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE > $OUT/pmc_$TAG.json
cat $OUT/pmc_$TAG.json
