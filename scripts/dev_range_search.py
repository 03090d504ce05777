"""Range search against top-k on the bench's index (GPU box): the pipeline-built 1 M codes, M = 8, 1000 queries, each
query's radius = its 100th-NN distance (just above it, so the 100th and its ties are in).

Prints one JSON line: the synchronous range_search call next to a synchronous query_batch(top_k=100) on the same
queries (median of --reps calls each, alternating), results per query (mean, max) and the overflow reruns.  Kernel
times of range_count_kernel / range_emit_kernel: run it again under `rocprofv3 --kernel-trace --stats -- python ...`
with --reps 5.
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

with api.DeltaPQIndex.open_memory(payload, args.n, 8, 256) as idx:
    idx.set_codebook(cb)
    ids, dists = idx.query_batch(queries, args.k)
    radii = np.nextafter(dists[:, -1], np.float32(np.inf))
    lims, rids, rd = idx.range_search(queries, radii)          # warm-up (allocations)
    counts = np.diff(lims)
    assert np.all(counts >= args.k)
    assert all(np.array_equal(rids[lims[q]:lims[q] + args.k], ids[q]) for q in range(args.queries))
    idx.profile_reset()
    idx.profile_enable(True)
    idx.range_search(queries, radii)
    prof = idx.profile_read()
    idx.profile_enable(False)
    t_range, t_topk = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        idx.range_search(queries, radii)
        t_range.append(time.perf_counter() - t)
        t = time.perf_counter()
        idx.query_batch(queries, args.k)
        t_topk.append(time.perf_counter() - t)

r_ms, k_ms = 1e3 * float(np.median(t_range)), 1e3 * float(np.median(t_topk))
print(json.dumps({
    "n": args.n, "queries": args.queries, "radius": "nextafter(%d-th NN distance)" % args.k, "reps": args.reps,
    "range_search_ms": round(r_ms, 3), "query_batch_top%d_ms" % args.k: round(k_ms, 3), "ratio": round(r_ms / k_ms, 3),
    "results_per_query_mean": float(counts.mean()), "results_per_query_max": int(counts.max()),
    "overflow_reruns": prof["overflow_reruns"], "profiled_call": {k: prof[k] for k in ("scan_ms", "select_ms", "lut_ms",
                                                                                         "quantise_ms", "decode_ms",
                                                                                         "scan_launches", "exact_checks",
                                                                                         "candidates")},
    "setup_s": round(setup_s, 1)}), flush=True)
