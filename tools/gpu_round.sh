#!/bin/bash
# One GPU-box visit: parity tests, smoke, short bench.  Everything is logged under $OUT/.
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
echo "== rocm-smi ==" > $OUT/env.log; rocm-smi --showproductname 2>&1 | head -20 >> $OUT/env.log; nproc >> $OUT/env.log; free -g >> $OUT/env.log
timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $OUT/pytest_gpu.log
tail -60 $OUT/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log; tail -8 $OUT/smoke.log
if [ "$1" == "bench" ]; then
  timeout 900 python bench.py --full --steps ${2:-10} --warmup 2 > $OUT/bench.log 2>&1; echo "bench exit $?" >> $OUT/bench.log; tail -12 $OUT/bench.log
fi
