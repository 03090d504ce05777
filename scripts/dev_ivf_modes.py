#!/usr/bin/env python
"""Measurements of the IVF search with a filter, by inner product and by radius on the bench-shaped
vectors; prints one JSON line and asserts nothing.

nlist centroids from a torch k-means over the base, lists by the nearest centroid of every node's original vector
(dev_ivf_search.py's second structure).  Per nprobe, ms per synchronous call, the calls of a row taking turns, median
[min - max] of `--reps` rounds:
  filter   search_torch under a filter that allows 100 % / 10 % / 0.1 % of the ids, beside the unfiltered search_torch
           and query_batch_filtered_torch under the same filter;
  ip       search_ip_torch beside query_batch_ip_torch;
  range    range_search at the median 100th-neighbour radius beside DeltaPQIndex.range_search (host forms both).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deltapq_amd import api, synth  # noqa: E402
from dev_candidate_search import taking_turns  # noqa: E402
from dev_ivf_search import kmeans, nearest  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--kmeans-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    n, k, nlist = args.n, args.topk, args.nlist
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, kmeans_iters=args.kmeans_iters)
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    d_base = torch.from_numpy(base).cuda()
    cents_t = kmeans(d_base, nlist, args.kmeans_iters, 3)
    cents = cents_t.cpu().numpy()
    labels = nearest(d_base, cents_t).to(torch.int32)[torch.from_numpy(tree.vec_id.astype(np.int64)).cuda()].contiguous()
    del d_base
    rng = np.random.default_rng(5)
    with api.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        d_q = torch.from_numpy(qs).cuda()
        radius = float(np.median(idx.query_batch(qs, k)[1][:, k - 1]))
        out["radius"] = radius
        with api.IVF.from_labels(idx, labels, nlist, centroids=cents) as ivf:
            filters = {}
            for name, frac in (("100", 1.0), ("10", 0.1), ("0.1", 0.001)):
                mask = np.ones(n + 1, dtype=bool) if frac == 1.0 else rng.random(n + 1) < frac
                filters[name] = api.IdFilter.from_mask(idx, mask)
            for nprobe in args.nprobe:
                row = {}
                for name, f in filters.items():
                    fns = {"ivf_search_filtered": lambda: ivf.search_torch(d_q, nprobe, k, id_filter=f),
                           "ivf_search": lambda: ivf.search_torch(d_q, nprobe, k),
                           "query_batch_filtered": lambda: idx.query_batch_filtered_torch(d_q, k, f)}
                    row["filter_%s_percent" % name] = dict(call_ms=taking_turns(fns, args.reps), n_allowed=f.n_allowed)
                fns = {"ivf_search_ip": lambda: ivf.search_ip_torch(d_q, nprobe, k),
                       "query_batch_ip": lambda: idx.query_batch_ip_torch(d_q, k)}
                got = ivf.search_ip_torch(d_q, nprobe, k)[0].cpu().numpy()
                row["ip"] = dict(call_ms=taking_turns(fns, args.reps),
                                 recall_vs_exhaustive_ip=api.recall(got, idx.query_batch_ip_torch(d_q, k)[0].cpu().numpy()))
                fns = {"ivf_range_search": lambda: ivf.range_search(qs, nprobe, radius),
                       "range_search": lambda: idx.range_search(qs, radius)}
                lims = ivf.range_search(qs, nprobe, radius)[0]
                row["range"] = dict(call_ms=taking_turns(fns, args.reps), results_per_query=float(lims[-1]) / args.nq,
                                    exhaustive_results_per_query=float(idx.range_search(qs, radius)[0][-1]) / args.nq)
                out["nprobe_%d" % nprobe] = row
            for f in filters.values():
                f.close()
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
