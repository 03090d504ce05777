#!/bin/bash
export RESULTS=${RESULTS:-results}   # where this script writes, relative to the repository root
export DPQ_DEV=1   # developer switches of the library are read only with this set
mkdir -p $RESULTS
for cap in 3072 4096 6144 3072 4096 6144; do
DPQ_BOOT_CAP=$cap python bench.py --full --no-cpu-baseline --reps 5 > $RESULTS/bc.json 2>$RESULTS/bc.err || { tail -5 $RESULTS/bc.err; exit 1; }
python - <<PY
import json
d=json.loads(open("$RESULTS/bc.json").read().strip().splitlines()[-1])
r=d["roofline"]
print("cap $cap", round(d["value"]), round(d["ms_per_step"],4), "scan", round(r["scan_ms_per_step"],4), "boot+sel", round(r["select_ms_per_step"],4), "checks/q", round(r["filter_survivors_per_query"]), "cand/q", round(r["candidates_per_query"]), flush=True)
PY
done
