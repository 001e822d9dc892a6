#!/bin/bash
# iteration visit: gpu tests + kernel microbench + short bench
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
timeout 900 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1; echo "pytest exit $?" >> $OUT/pytest_gpu.log; tail -25 $OUT/pytest_gpu.log
timeout 600 python tools/bench_kernels.py $MICRO > $OUT/micro.log 2>&1; cat $OUT/micro.log | grep -v amdgpu.ids
if [ -n "$MICRO2ENV" ]; then env $MICRO2ENV timeout 600 python tools/bench_kernels.py $MICRO2 > $OUT/micro2.log 2>&1; cat $OUT/micro2.log | grep -v amdgpu.ids; fi
timeout 600 python bench.py --full --steps 20 --warmup 3 --no-cpu-baseline > $OUT/bench_iter.log 2>&1; tail -1 $OUT/bench_iter.log | cut -c1-150
