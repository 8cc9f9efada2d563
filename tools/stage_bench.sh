#!/bin/bash
# full-table stages only; prints stages_ms
OUT=${BENCH_OUT_DIR:-/tmp}      # where the line and the log go
python bench.py --full --no-cpu --no-e2e "$@" > "$OUT/sb.json" 2> "$OUT/sb.err" || tail -5 "$OUT/sb.err"
python - <<PY
import json
d = json.loads(open("$OUT/sb.json").read().strip().splitlines()[-1])
ft = d.get("full_table") or d["config"].get("full_table")
print("full", ft["ms_per_frame"], "frac", ft["frac"], ft["stages_ms"], ft["parity"][:30])
PY
