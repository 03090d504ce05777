"""Filtered top-k search against unfiltered top-k on the bench's index (GPU box): the pipeline-built 1 M codes, M = 8,
1000 queries, top-100.

Prints one JSON line: per selectivity (100 / 50 / 10 / 1 / 0.1 % of the ids, a seeded random mask) the synchronous
query_batch_filtered call next to a synchronous query_batch on the same queries (median of --reps calls each,
alternating), the same for one query (nq = 1: the stream pass unfiltered, one filter-scan query group filtered), and per
selectivity one profiled call's exact checks, candidates and overflow reruns per query.  Kernel times: run it again
under `rocprofv3 --kernel-trace --stats -- python ...` with --reps 5.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from deltapq_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()

t0 = time.time()
base = synth.make_clustered_vectors(args.n, 128, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
cb = synth.kmeans_codebook(base, 8, 256, iters=6, seed=102)
codes = api.encode_pq(base, cb)
del base
tree = api.DeltaTree(codes, codebook=cb, device=0)
payload = tree.payload()
tree.close()
queries = synth.make_clustered_vectors(args.queries, 128, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
setup_s = time.time() - t0


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


out = {"n": args.n, "queries": args.queries, "k": args.k, "reps": args.reps, "selectivity": {}}
with api.DeltaPQIndex.open_memory(payload, args.n, 8, 256) as idx:
    idx.set_codebook(cb)
    ref = idx.query_batch(queries, args.k)
    for frac in (1.0, 0.5, 0.1, 0.01, 0.001):
        mask = np.ones(args.n + 1, dtype=bool) if frac == 1.0 else np.random.default_rng(7).random(args.n + 1) < frac
        with api.IdFilter.from_mask(idx, mask) as f:
            got = idx.query_batch_filtered(queries, args.k, f)          # warm-up (allocations, plan)
            if frac == 1.0:
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
            idx.profile_reset()
            idx.profile_enable(True)
            idx.query_batch_filtered(queries, args.k, f)
            prof = idx.profile_read()
            idx.profile_enable(False)
            allowed = f.n_allowed
            t_f, t_u, t_f1, t_u1 = [], [], [], []
            for _ in range(args.reps):
                t_f.append(timed(lambda: idx.query_batch_filtered(queries, args.k, f)))
                t_u.append(timed(lambda: idx.query_batch(queries, args.k)))
                t_f1.append(timed(lambda: idx.query_batch_filtered(queries[:1], args.k, f)))
                t_u1.append(timed(lambda: idx.query_batch(queries[:1], args.k)))
        f_ms, u_ms = 1e3 * float(np.median(t_f)), 1e3 * float(np.median(t_u))
        f1_ms, u1_ms = 1e3 * float(np.median(t_f1)), 1e3 * float(np.median(t_u1))
        nq = max(1, prof["queries"])
        out["selectivity"]["%g%%" % (100 * frac)] = {
            "allowed": allowed,
            "filtered_ms": round(f_ms, 3), "unfiltered_ms": round(u_ms, 3), "ratio": round(f_ms / u_ms, 3),
            "nq1_filtered_ms": round(f1_ms, 3), "nq1_unfiltered_ms": round(u1_ms, 3),
            "exact_checks_per_query": round(prof["exact_checks"] / nq, 1),
            "candidates_per_query": round(prof["candidates"] / nq, 1),
            "overflow_reruns_per_query": round(prof["overflow_reruns"] / nq, 4),
            "profiled_call": {k: prof[k] for k in ("scan_ms", "select_ms", "lut_ms", "bootstrap_ms", "quantise_ms",
                                                   "decode_ms", "scan_launches")}}
out["setup_s"] = round(setup_s, 1)
print(json.dumps(out), flush=True)
