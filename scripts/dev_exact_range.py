#!/usr/bin/env python
"""How good DeltaPQIndex.range_search is, held against the exact FlatIndex.range_search, on the vectors
of dev_exact_search.py; prints one JSON line.

The radius is the median exact `--topk`-th-neighbour distance of the queries.  The exact answer is timed (`--reps` calls,
host buffers in and out) without a filter and under a random 10 % filter; the PQ answer (train, encode, DeltaTree, one
radius for every query: the PQ distances are approximations of the exact ones) is mapped from DFS positions to vector
ids and scored with range_recall: recall and precision summed over the queries.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deltapq_amd import api, synth  # noqa: E402


def spread(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    n = args.n
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=args.topk, reps=args.reps)
    with api.FlatIndex(base) as flat:
        (_, kd), out["search_call_ms"] = timed(lambda: flat.search(qs, args.topk), args.reps)
        radius = float(np.median(kd[:, -1]))
        out["radius"] = radius
        truth, out["range_search_call_ms"] = timed(lambda: flat.range_search(qs, radius), args.reps)
        out["exact_entries"] = int(truth[0][-1])
        out["exact_longest_list"] = int(np.diff(truth[0]).max())
        mask = np.random.default_rng(103).random(n) < 0.1
        with api.FlatIdFilter.from_mask(flat, mask) as ff:
            tf, out["range_search_10pct_filter_call_ms"] = timed(lambda: flat.range_search(qs, radius, ff), args.reps)
        out["exact_entries_10pct_filter"] = int(tf[0][-1])
        inf, out["range_search_inf_8_queries_call_ms"] = timed(lambda: flat.range_search(qs[:8], np.inf), args.reps)
        assert int(inf[0][-1]) == 8 * n
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    with api.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        (lims, pos, _), out["pq_range_search_call_ms"] = timed(lambda: idx.range_search(qs, radius), args.reps)
    p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    found = tree.vec_id[p].astype(np.int32)
    out["pq_entries"] = int(lims[-1])
    out["pq_range_recall"], out["pq_range_precision"] = api.range_recall((lims, found), truth)
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
