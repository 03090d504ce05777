"""Randomised parity stress: HIP path vs oracle over random shapes/options (GPU box).  Every case is drawn by
tests/_option_matrix.py (draw_case: the axes of tests/test_option_matrix.py, with sizes of this script's own) and goes
through its call sequence on every handle -- unfiltered top-k, filtered top-k under three masks, range search over the
six radius kinds, code lookup of the filtered rows, the unfiltered call again -- against its numpy references over the
oracle's per-code distances; sharded cases also merged.  A developer script, not part of the suite.
usage: python scripts/fuzz_parity.py [seconds] [seed]     (DPQ_FUZZ_BIG=1: also shards of up to 400 K nodes)"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _option_matrix as om
from deltapq_amd import api
from oracle import dtc_oracle as O

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
orc = O.Oracle()
t_end = time.time() + budget
cases = bad = 0
while time.time() < t_end:
    n = int(rng.choice([1, 2, 3, 63, 64, 65, 255, 257, int(rng.integers(300, 3000)), int(rng.integers(3000, 60000))]))
    if os.environ.get("DPQ_FUZZ_BIG") == "1" and rng.random() < 0.3:
        n = int(rng.integers(17000, 400000))  # bootstrap shards
    c = om.draw_case(rng, n=n)
    if om.n_eff(c) * c["nq"] > 20_000_000:    # the references hold every distance of every query
        c["nq"] = 33
    try:
        om.run_case(api, orc, c)
    except AssertionError as e:
        bad += 1
        print("MISMATCH %s: %s" % (om.case_id(c), str(e).splitlines()[0]), flush=True)
    except Exception as e:   # noqa: BLE001
        bad += 1
        print("ERROR %s: %r" % (om.case_id(c), e), flush=True)
        cases += 1
        break                # a library or HIP error: start nothing more on this GPU
    cases += 1
    if cases % 25 == 0:
        print("%d cases, %d bad" % (cases, bad), flush=True)
print("FUZZ DONE: %d cases, %d bad" % (cases, bad))
sys.exit(1 if bad else 0)
