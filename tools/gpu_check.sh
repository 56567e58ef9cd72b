#!/bin/bash
# GPU suite, smoke, the full bench line (no CPU leg) and the per-rank
# stripe step table; logs under $OUT (default check_out/).
OUT=${OUT:-check_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/gputest.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -4 $OUT/gputest.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { cat $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
timeout -k 10 300 python bench.py --full --no-cpu ${BENCH_ARGS} 2>$OUT/bench.err | tail -1 > $OUT/bench.json || exit 1
cat $OUT/bench.json
timeout -k 10 300 python tools/exp_stripes.py 50 20 > $OUT/stripes.jsonl 2>$OUT/stripes.err || exit 1
cat $OUT/stripes.jsonl
