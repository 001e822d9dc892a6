#!/bin/bash
# round-5 check visit: the whole -m gpu suite with its printed margins (not -x: every failure is listed), then the driver-style bench line
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
TAG=${1:-r05a}
timeout 1500 python -m pytest tests -m gpu -q -s --tb=short -p no:cacheprovider > $OUT/pytest_$TAG.log 2>&1; echo "pytest exit $?" >> $OUT/pytest_$TAG.log
grep -a "passed\|failed\|FAILED\|ERROR\|pytest exit" $OUT/pytest_$TAG.log | tail -30
if [ -z "$NO_BENCH" ]; then
  timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_${TAG}_20.log 2>&1; echo "bench20 exit $?"; tail -1 $OUT/bench_${TAG}_20.log | cut -c1-400
fi
