#!/bin/bash
# The GPU suite and one full bench line, with the figures worth a glance.   bash tools/_health.sh <out dir>
OUT=${1:?usage: bash tools/_health.sh <out dir>}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT/gpu_suite.log" 2>&1; echo "pytest rc=$?"
tail -5 "$OUT/gpu_suite.log"
( time python bench.py --full > "$OUT/bench_line.json" 2> "$OUT/bench.err" ) 2>&1 | tail -4
python - "$OUT/bench_line.json" <<'PY'
import json, sys
j=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(j['value'], j['ms_per_step'], j['roofline'].get('frac'))
print(json.dumps(j.get('c4_sharded'))[:1500])
print(json.dumps(j.get('dropin_loop'))[:800])
print(json.dumps(j.get('c3_engine'))[:800])
print(j.get('regressions'))
PY
