#!/bin/bash
# M = 16 filter geometry sweep: libraries built with -DDPQ_PRE16/-DDPQ_SAT16/-DDPQ_QT16 under variants/
export RESULTS=${RESULTS:-results}   # where this script writes, relative to the repository root
mkdir -p $RESULTS
for lib in variants/lib_*.so; do
  for k in 1000 100; do
    DPQ_LIB_PATH=$PWD/$lib python bench.py --full --no-cpu-baseline --reps 3 --m 16 --topk $k > $RESULTS/sweep.json 2>$RESULTS/sweep.err || { tail -5 $RESULTS/sweep.err; continue; }
    python - <<PY
import json
d=json.loads(open("$RESULTS/sweep.json").read().strip().splitlines()[-1])
r=d["roofline"]
print("$lib top$k", round(d["value"]), round(d["ms_per_step"],4), "scan", round(r["scan_ms_per_step"],4), "checks/q", round(r["filter_survivors_per_query"]), "cand/q", round(r["candidates_per_query"]), flush=True)
PY
  done
done 2>&1 | tee $RESULTS/m16_sweep.txt
