#!/bin/bash
# Runs ON THE GPU BOX (via gpurun): per-launch durations of the query-path kernels of the last bench steps.
export RESULTS=${RESULTS:-results}   # where this script writes, relative to the repository root
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
rm -rf $RESULTS/kt
timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d $RESULTS/kt -- python bench.py --full --steps 3 --warmup 1 --check 0 --no-cpu-baseline "$@" > /dev/null 2> $RESULTS/kt.err
python - <<'PY'
import csv, glob, os
f = glob.glob(os.environ["RESULTS"] + "/kt/*/*_kernel_trace.csv")[0]
rows = [r for r in csv.DictReader(open(f)) if "dpq::s" in r["Kernel_Name"] or "lut_build" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
for r in rows[-8:]:
    print("%-28s %7.1f us" % (r["Kernel_Name"].split("(")[0][-28:], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
PY
rm -rf $RESULTS/kt
