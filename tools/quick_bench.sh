#!/bin/bash
# quick: headline only; prints value, ms, kernel table
OUT=${BENCH_OUT_DIR:-/tmp}      # where the line and the log go
python bench.py --full --no-cpu --no-full --no-e2e "$@" > "$OUT/qb.json" 2> "$OUT/qb.err" || tail -5 "$OUT/qb.err"
python - <<PY
import json
d = json.loads(open("$OUT/qb.json").read().strip().splitlines()[-1])
print("value", d["value"], "ms", d["ms_per_step"], "dom", d["roofline"]["kernel"], d["roofline"]["frac"], "path", d["roofline"]["path"]["frac"], d["config"]["parity"][:20])
print(d["roofline"]["kernels_ms"])
PY
