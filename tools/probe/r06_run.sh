#!/bin/bash
# scratch: run on the GPU box
OUT=${CD360_OUT:-/tmp/cd360_out}; mkdir -p $OUT
python -c "import __graft_entry__ as g; g.build(); g.smoke(); print('smoke ok')" 2>&1 | tail -1
timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider > $OUT/pytest_r06i.log 2>&1; echo "pytest exit $?" >> $OUT/pytest_r06i.log; grep -a "passed\|failed\|pytest exit" $OUT/pytest_r06i.log | tail -3
python bench.py --full --steps 20 --warmup 5 2>/dev/null | tail -1 > $OUT/bench_r06i_20.json; python -c "
import json; d=json.load(open('$OUT/bench_r06i_20.json')); print(d['value'], d['ms_per_step'], d['config']['steady_step_ms'], d['config']['render_step_ms'], d['roofline']['frac'])"
