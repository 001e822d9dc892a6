#!/bin/bash
# round-5 evidence pass, one box: rocprofv3 kernel trace + PMC passes (tools/gpu_profile.sh), ONE steady step by kernel -- eager AND as the
# hipGraph replay the bench times --, the fine-tune step by kernel as the graph replay, SQ counters of the fused attention, bench lines
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
TAG=${1:-r05a}
cd $ROOT
timeout 1500 python -m pytest tests -m gpu -q -s --tb=short -p no:cacheprovider > $OUT/pytest_$TAG.log 2>&1; echo "pytest exit $?" >> $OUT/pytest_$TAG.log; grep -a "passed\|failed\|pytest exit" $OUT/pytest_$TAG.log | tail -5
bash tools/gpu_profile.sh $TAG 6 > $OUT/evidence_$TAG.log 2>&1
bash tools/gpu_steady_diff.sh $TAG >> $OUT/evidence_$TAG.log 2>&1
STEADY_NOGRAPH=" " bash tools/gpu_steady_diff.sh ${TAG}_graph >> $OUT/evidence_$TAG.log 2>&1
TRAIN_ARGS=--graph bash tools/gpu_steady_diff_train.sh ${TAG}_graph 1 5 >> $OUT/evidence_$TAG.log 2>&1
bash tools/gpu_pmc_qattn.sh $TAG - > /dev/null 2>&1
timeout 900 python bench.py --full --steps 20 --warmup 5 > $OUT/bench_${TAG}_20.log 2>&1; echo "bench20 exit $?"; tail -1 $OUT/bench_${TAG}_20.log | cut -c1-200
timeout 900 python bench.py --full > $OUT/bench_${TAG}_default.log 2>&1; echo "bench exit $?"; tail -1 $OUT/bench_${TAG}_default.log | cut -c1-200
timeout 900 python bench.py --full --steps 20 --warmup 5 --fp8-attn --no-train-step --no-cpu-baseline > $OUT/bench_${TAG}_fp8.log 2>&1; echo "bench fp8 exit $?"
timeout 900 python bench.py --full --steps 20 --warmup 5 --poses 2 --poses-per-replay 2 --no-train-step --no-cpu-baseline > $OUT/bench_${TAG}_ppr2.log 2>&1; echo "bench ppr2 exit $?"
grep -a "exit\|steady step\|fine-tune step" $OUT/evidence_$TAG.log
timeout 900 python bench.py --full --steps 20 --warmup 5 --route sample_py --no-train-step --no-cpu-baseline > $OUT/bench_${TAG}_sample_py.log 2>&1; echo "bench sample_py exit $?"
timeout 900 python bench.py --steps 20 --warmup 5 --route module --no-train-step --no-cpu-baseline --no-profile > $OUT/bench_${TAG}_module.log 2>&1; echo "bench module exit $?"
for f in 20 default fp8 ppr2 sample_py module; do tail -1 $OUT/bench_${TAG}_$f.log | python -c "
import json,sys
try:
    d=json.loads(sys.stdin.read()); c=d['config']; print('$f: %.2f steps/s steady %.2f render %.2f train %s' % (d['value'], c['steady_step_ms'], c['render_step_ms'], d.get('train_step',{}).get('ms')))
except Exception as e: print('$f: no line', e)"; done
