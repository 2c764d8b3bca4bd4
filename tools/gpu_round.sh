#!/bin/bash
# usage (on the GPU box): tools/gpu_round.sh <tag> [tests|bench|prof]...
# Each GPU step has its own time limit; the script stops at the first failure.  Logs and results go to $OUT
# (default bench_out/, git-ignored).
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}
TAG=$1; shift
mkdir -p $OUT
for step in "$@"; do
  case $step in
    tests)
      timeout -k 10 1150 python -u -m pytest tests -m gpu -x -v --durations=40 --timeout 600 --timeout-method thread \
        > $OUT/tests_$TAG.log 2>&1 || { echo "tests failed"; tail -30 $OUT/tests_$TAG.log; exit 1; } ;;
    bench)
      timeout -k 10 600 python -u bench.py --full --steps 10 --warmup 3 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err \
        || { echo "bench failed"; tail -30 $OUT/bench_$TAG.err; exit 1; }
      head -c 2500 $OUT/bench_$TAG.json ;;
    prof)
      timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv \
        -- python3 bench.py --full --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 \
        || { echo "prof failed"; tail -30 $OUT/prof_$TAG.log; exit 1; }
      find $OUT/prof_$TAG -name "*kernel_stats.csv" -exec cp {} $OUT/prof_$TAG.kernel_stats.csv \;
      head -25 $OUT/prof_$TAG.kernel_stats.csv ;;
    configs|configs:*)  # the other BASELINE shapes on one GPU, each with its CPU baseline (a bounded sample where the
      # full run is too long; bench.py CPU_SAMPLE_SCALE).  configs:<cfg>@<scale>,... picks them
      LIST="c1@1.0 c3@0.5 c3@1.0 c4@0.05 c4@0.4 c5@0.1 c5@0.3"
      [ "$step" != configs ] && LIST=$(echo "${step#configs:}" | tr ',' ' ')
      for cs in $LIST; do
        CFG=${cs%@*}; SC=${cs#*@}
        echo "config $CFG scale $SC" >&2
        timeout -k 10 500 python -u bench.py --full --config $CFG --scale $SC --steps 3 --warmup 1 --no-ingest \
          > $OUT/cfg_${TAG}_${CFG}_$SC.json 2> $OUT/cfg_${TAG}_${CFG}_$SC.err \
          || { echo "config $CFG $SC failed"; tail -20 $OUT/cfg_${TAG}_${CFG}_$SC.err; exit 1; }
        head -c 600 $OUT/cfg_${TAG}_${CFG}_$SC.json; echo
      done ;;
    cprof:*)  # cprof:<config>:<scale> -- kernel stats of one step of another BASELINE shape
      IFS=: read -r _ CFG SC <<< "$step"
      timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/cprof_${TAG}_$CFG -o run --output-format csv \
        -- python3 bench.py --full --config $CFG --scale $SC --steps 2 --warmup 1 --no-cpu-baseline --no-ingest \
        > $OUT/cprof_${TAG}_$CFG.log 2>&1 \
        || { echo "cprof $CFG failed"; tail -30 $OUT/cprof_${TAG}_$CFG.log; exit 1; }
      find $OUT/cprof_${TAG}_$CFG -name "*kernel_stats.csv" -exec cp {} $OUT/cprof_${TAG}_$CFG.kernel_stats.csv \;
      cut -c1-60,200- $OUT/cprof_${TAG}_$CFG.kernel_stats.csv | head -30 ;;
    qprof)
      timeout -k 10 300 rocprofv3 --kernel-trace -d $OUT/qprof_$TAG -o run --output-format csv \
        -- python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 1 > $OUT/qprof_$TAG.log 2>&1 \
        || { echo "qprof failed"; tail -30 $OUT/qprof_$TAG.log; exit 1; }
      python3 tools/trace_step.py $OUT/qprof_$TAG/run_kernel_trace.csv | awk '$2 > 40 || /total/' ;;
    pmc)
      tools/pmc.sh $TAG || exit 1 ;;
    pmc:*)  # pmc:<config>:<scale> -- the PMC passes on another BASELINE shape
      IFS=: read -r _ CFG SC <<< "$step"
      tools/pmc.sh ${TAG}_$CFG --config $CFG --scale $SC || exit 1 ;;
    lstats)
      timeout -k 10 300 python -u tools/light_stats.py c2 1.0 > $OUT/lstats_$TAG.log 2>&1 \
        || { echo "lstats failed"; tail -30 $OUT/lstats_$TAG.log; exit 1; }
      grep LIGHT_STATS $OUT/lstats_$TAG.log ;;
    quick)
      timeout -k 10 300 python -u tools/gpu_quick.py > $OUT/quick_$TAG.log 2>&1 \
        || { echo "quick failed"; tail -30 $OUT/quick_$TAG.log; exit 1; }
      tail -5 $OUT/quick_$TAG.log ;;
    distinct)
      timeout -k 10 300 python -u tools/distinct_bench.py > $OUT/distinct_$TAG.log 2>&1 \
        || { echo "distinct failed"; tail -30 $OUT/distinct_$TAG.log; exit 1; }
      timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/dprof_$TAG -o run --output-format csv \
        -- python3 tools/distinct_bench.py > $OUT/dprof_$TAG.log 2>&1 \
        || { echo "distinct prof failed"; tail -30 $OUT/dprof_$TAG.log; exit 1; }
      find $OUT/dprof_$TAG -name "*kernel_stats.csv" -exec cp {} $OUT/dprof_$TAG.kernel_stats.csv \;
      grep DISTINCT $OUT/distinct_$TAG.log; grep distinct $OUT/dprof_$TAG.kernel_stats.csv | cut -c1-40,150- ;;
    parse)
      timeout -k 10 400 python -u tools/parse_bench.py > $OUT/parse_$TAG.log 2>&1 \
        || { echo "parse failed"; tail -30 $OUT/parse_$TAG.log; exit 1; }
      grep -E "PARSE|text" $OUT/parse_$TAG.log ;;
    pprof)
      timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/pprof_$TAG -o run --output-format csv \
        -- python3 tools/parse_bench.py > $OUT/pprof_$TAG.log 2>&1 \
        || { echo "parse prof failed"; tail -30 $OUT/pprof_$TAG.log; exit 1; }
      find $OUT/pprof_$TAG -name "*kernel_stats.csv" -exec cp {} $OUT/pprof_$TAG.kernel_stats.csv \;
      grep -E "k_nt|scan" $OUT/pprof_$TAG.kernel_stats.csv | cut -c1-40,150- ;;
    rehearse:*)  # rehearse:<config>:<scale>:<ranks> -- sharded bench with several ranks on the one GPU (gloo)
      IFS=: read -r _ CFG SC NR <<< "$step"
      tools/shard_rehearsal.sh ${TAG}_${CFG}_$NR $CFG $SC $NR || exit 1 ;;
    tfile:*)  # tfile:<test file>[,<test file>...][@-k expr] -- GPU test files (one pytest process), with a heartbeat
      SPEC=${step#tfile:}; FILES=$(echo "${SPEC%%@*}" | tr ',' ' '); KEXPR=""
      [[ "$SPEC" == *@* ]] && KEXPR="${SPEC#*@}"
      timeout -k 10 1000 python -u -m pytest $FILES -m gpu -x -v --timeout 600 --timeout-method thread ${KEXPR:+-k "$KEXPR"} \
        > $OUT/tfile_$TAG.log 2>&1 &
      PID=$!
      while kill -0 $PID 2>/dev/null; do sleep 30; echo "[hb $(date +%T)] $(grep -cE 'PASSED' $OUT/tfile_$TAG.log) passed"; done
      wait $PID || { echo "tfile failed"; tail -60 $OUT/tfile_$TAG.log; exit 1; }
      grep -cE "PASSED" $OUT/tfile_$TAG.log; tail -2 $OUT/tfile_$TAG.log ;;
    benchcfg:*)  # benchcfg:<config>:<scale>:<steps> -- one BASELINE shape on one GPU, with a heartbeat (long steps)
      IFS=: read -r _ CFG SC NS <<< "$step"
      timeout -k 10 1000 python -u bench.py --config $CFG --scale $SC --steps $NS --warmup 0 --no-cpu-baseline --no-ingest --no-resident --page-log \
        > $OUT/bcfg_${TAG}_$CFG.json 2> $OUT/bcfg_${TAG}_$CFG.err &
      PID=$!
      while kill -0 $PID 2>/dev/null; do sleep 30; echo "[hb $(date +%T)] $(tail -c 200 $OUT/bcfg_${TAG}_$CFG.err | tr '\n' ' ')"; done
      wait $PID || { echo "benchcfg $CFG failed"; tail -30 $OUT/bcfg_${TAG}_$CFG.err; exit 1; }
      cat $OUT/bcfg_${TAG}_$CFG.json ;;
    gtest:*)  # gtest:<pytest -k expression> -- a subset of the GPU tests
      timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -k "${step#gtest:}" \
        > $OUT/gtest_$TAG.log 2>&1 || { echo "gtest failed"; tail -30 $OUT/gtest_$TAG.log; exit 1; }
      tail -3 $OUT/gtest_$TAG.log ;;
    *) echo "unknown step $step"; exit 2 ;;
  esac
done
echo "all steps ok"
