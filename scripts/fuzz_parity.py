"""Randomised parity stress: HIP path vs oracle over random shapes/options (GPU box).  Every case is drawn by
tests/_option_matrix.py (draw_case: the axes of tests/test_option_matrix.py, with sizes of this script's own) and goes
through its call sequence on every handle -- unfiltered top-k, filtered top-k under three masks, range search over the
six radius kinds, code lookup of the filtered rows, the unfiltered call again -- against its numpy references over the
oracle's per-code distances; sharded cases also merged.  A developer script, not part of the suite.
usage: python scripts/fuzz_parity.py [seconds] [seed] [--tables synth|all|CLASS]     (DPQ_FUZZ_BIG=1: also shards of up to 400 K nodes)
--tables: where codebook, queries and tree come from.  synth (the default): synth.make_codebook / make_queries, as ever.
A class of tests/_numeric_edges.py (zero_threshold, constant, ulp_crowd, fp32_ties, ladder_low / mid / high, tiny_gaussian,
overflow) or `all` (one drawn per case): its Ds = 1 codebook on the dyadic grid, its four queries in turn and its tree at the
case's n, M and K -- the random option draws crossed with the numeric edges."""
import argparse, sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _option_matrix as om
import _numeric_edges as ne
from deltapq_amd import api, synth
from oracle import dtc_oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("seconds", nargs="?", type=float, default=120.0)
ap.add_argument("seed", nargs="?", type=int, default=0)
ap.add_argument("--tables", default="synth", choices=["synth", "all"] + list(ne.CLASSES))
args = ap.parse_args()
budget = args.seconds
rng = np.random.default_rng(args.seed)


def class_inputs(c, name):
    """om.build_inputs with codebook, queries and tree of a numeric-edge class (Ds = 1)."""
    c["Ds"] = 1
    k = ne.CLASSES[name](c["M"], c["K"], c["n"], seed=c["seed"])
    payload, _ = synth.encode_dtc(k["tree"])
    qs = np.ascontiguousarray(k["queries"][np.arange(c["nq"]) % len(k["queries"])])
    return dict(cb=k["cb"], tree=k["tree"], payload=payload, qs=qs, codes=synth.decode_tree_codes(k["tree"]))


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
    name = args.tables if args.tables != "all" else list(ne.CLASSES)[int(rng.integers(len(ne.CLASSES)))]
    what = om.case_id(c) if name == "synth" else "%s %s" % (name, om.case_id(c))
    try:
        om.run_case(api, orc, c, inp=None if name == "synth" else class_inputs(c, name))
    except AssertionError as e:
        bad += 1
        print("MISMATCH %s: %s" % (what, str(e).splitlines()[0]), flush=True)
    except Exception as e:   # noqa: BLE001
        bad += 1
        print("ERROR %s: %r" % (what, e), flush=True)
        cases += 1
        break                # a library or HIP error: start nothing more on this GPU
    cases += 1
    if cases % 25 == 0:
        print("%d cases, %d bad" % (cases, bad), flush=True)
print("FUZZ DONE: %d cases, %d bad" % (cases, bad))
sys.exit(1 if bad else 0)
