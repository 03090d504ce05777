#!/bin/bash
export RESULTS=${RESULTS:-results}   # where this script writes, relative to the repository root
export DPQ_DEV=1
# bootstrap size against the in-scan tightening: how many nodes the bootstrap should evaluate now that the scan tightens by itself
mkdir -p $RESULTS
for cfg in "0 1" "2048 1" "2560 1" "4096 1" "0 0" "2048 0"; do
set -- $cfg
DPQ_BOOT_CAP=$1 DPQ_TIGHTEN=$2 python bench.py --full --no-cpu-baseline --reps 6 > $RESULTS/bc.json 2>$RESULTS/bc.err || { tail -5 $RESULTS/bc.err; continue; }
python - <<PY
import json
d=json.loads(open("$RESULTS/bc.json").read().strip().splitlines()[-1])
r=d["roofline"]
print("boot_cap $1 tighten $2:", round(d["value"]), "q/s", round(d["ms_per_step"],4), "ms/step scan", round(r["scan_ms_per_step"],4), "select+boot", round(r["select_ms_per_step"],4), "checks/q", round(r["filter_survivors_per_query"]), "cand/q", round(r["candidates_per_query"]), flush=True)
PY
done 2>&1 | tee $RESULTS/boot_cap_tight.txt
