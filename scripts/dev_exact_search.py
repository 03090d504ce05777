#!/usr/bin/env python
"""Measurements of the exact search on the bench-shaped vectors; prints one JSON line.

  search   `--reps` exact top-`--topk` searches of `--nq` queries over all `--n` vectors (dpq_flat_search, host buffers
           in and out), and the same search through the numpy restatement on one CPU core for `--cpu-queries`
           queries, scaled to `--nq`
  rerank   the chain a user runs: train, encode, DeltaTree, PQ top-`--rerank` batch (dpq_query_batch), exact re-rank of
           that answer to top-`--topk` (dpq_flat_rerank on host buffers, dpq_flat_rerank_device on device tensors),
           each `--reps` times; recall@topk of the PQ answer and of the re-ranked answer against the exact search
A `rocprofv3 --kernel-trace --stats` run of this script gives the per-kernel split.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
    ap.add_argument("--mode", choices=("search", "rerank", "all"), default="all")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rerank", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-queries", type=int, default=2)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=args.n, dim=args.dim, nq=args.nq, top_k=args.topk, reps=args.reps)
    with api.FlatIndex(base) as flat:
        (truth, truth_d), out["search_call_ms"] = timed(lambda: flat.search(qs, args.topk), args.reps)
        triples = float(args.n) * args.nq * args.dim
        out["search_triples_per_s"] = triples / (out["search_call_ms"]["median"] * 1e-3)
        if args.cpu_queries > 0:
            import _exact_restatement as X
            t0 = time.perf_counter()
            ci, cd = X.search(base, qs[:args.cpu_queries], args.topk)
            cpu_s = time.perf_counter() - t0
            out["restatement_cpu_s_scaled_to_nq"] = cpu_s / args.cpu_queries * args.nq
            out["restatement_agrees"] = bool(np.array_equal(ci, truth[:args.cpu_queries]) and
                                             np.array_equal(cd.view(np.uint32), truth_d[:args.cpu_queries].view(np.uint32)))
        if args.mode in ("rerank", "all"):
            import torch
            cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
            codes = api.encode_pq(base, cb)
            tree = api.DeltaTree(codes, codebook=cb, device=0)
            flat.set_id_map(tree.vec_id)
            with api.DeltaPQIndex.open_memory(tree.payload(), args.n, 8, 256, device=0) as idx:
                idx.set_codebook(cb)
                (pos, _), out["pq_top%d_call_ms" % args.rerank] = timed(lambda: idx.query_batch(qs, args.rerank), args.reps)
            (ri, rd), out["rerank_call_ms"] = timed(lambda: flat.rerank(qs, pos, args.topk), args.reps)
            d_q, d_c = torch.from_numpy(qs).cuda(), torch.from_numpy(pos).cuda()

            def on_device():
                r = flat.rerank_torch(d_q, d_c, args.topk)
                torch.cuda.synchronize()
                return r
            (ti, _), out["rerank_device_call_ms"] = timed(on_device, args.reps)
            out["rerank_variants_agree"] = bool(np.array_equal(ti.cpu().numpy(), ri))
            n = args.n
            p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
            found = tree.vec_id[p].astype(np.int32)
            out["pq_recall_at_%d" % args.topk] = api.recall(found, truth, k=args.topk, R=args.topk)
            out["reranked_recall_at_%d" % args.topk] = api.recall(ri, truth, k=args.topk, R=args.topk)
            out["pq_recall_1_at_%d" % args.rerank] = api.recall(found, truth, k=1, R=args.rerank)
            tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
