#!/bin/bash
# end-of-iteration visit: full gpu tests, smoke, distributed-launch sanity (1 rank), headline bench
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
timeout 1200 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1; echo "pytest exit $?" >> $OUT/pytest_gpu.log; tail -15 $OUT/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log; tail -6 $OUT/smoke.log
timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 1 --steps 6 --warmup 2 --no-cpu-baseline > $OUT/bench_dist1.log 2>&1; echo "dist1 exit $?"; tail -2 $OUT/bench_dist1.log | cut -c1-200
timeout 900 python bench.py --full > $OUT/bench_default.log 2>&1; echo "bench exit $?"; tail -1 $OUT/bench_default.log
