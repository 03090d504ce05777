#!/usr/bin/env python
"""Measurements of the residual re-ranking on the bench-shaped vectors; prints one JSON line.

The chain a user runs: train, encode, DeltaTree, open; build a refine level (dpq_refine_build); PQ top-`--cand` batch;
then, on the SAME candidate lists, the refined re-rank (dpq_refine_rerank_device) beside the exact re-rank over raw
vectors (dpq_flat_rerank_device), each `--reps` times; the fused call (dpq_query_batch_refined); recall@topk of the PQ
answer, the refined answer and the exactly re-ranked answer against the exact search; bytes per vector of each option.
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
    ap.add_argument("--cand", type=int, default=1000)
    ap.add_argument("--m2", type=int, default=0)
    ap.add_argument("--k2", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    n, k = args.n, args.topk
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, n_cand=args.cand, reps=args.reps)
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    with api.FlatIndex(base) as flat, api.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        truth, _ = flat.search(qs, k)
        flat.set_id_map(tree.vec_id)
        idx.set_codebook(cb)
        t0 = time.perf_counter()
        lvl = api.RefineLevel.build(idx, base, vec_id=tree.vec_id, M2=args.m2, K2=args.k2)
        out["build_s"] = time.perf_counter() - t0
        out["M2"], out["K2"] = lvl.M2, lvl.K2
        (pos, _), out["pq_top%d_call_ms" % args.cand] = timed(lambda: idx.query_batch(qs, args.cand), args.reps)
        d_q, d_c = torch.from_numpy(qs).cuda(), torch.from_numpy(pos).cuda()

        def sync(fn):
            def run():
                r = fn()
                torch.cuda.synchronize()
                return r
            return run
        (ri, _), out["refine_rerank_device_call_ms"] = timed(sync(lambda: lvl.rerank_torch(d_q, d_c, k)), args.reps)
        (fi, _), out["flat_rerank_device_call_ms"] = timed(sync(lambda: flat.rerank_torch(d_q, d_c, k)), args.reps)
        (qi, _), out["query_batch_refined_call_ms"] = timed(lambda: lvl.query_batch_refined(qs, args.cand, k), args.reps)
        out["fused_equals_two_calls"] = bool(np.array_equal(qi, ri.cpu().numpy()))

        def to_vec(p):
            p = np.where((p == n) & (n % 2 == 0), n - 1, p)
            return np.where(p >= 0, tree.vec_id[np.maximum(p, 0)].astype(np.int64), -1).astype(np.int32)
        out["pq_recall_at_%d" % k] = api.recall(to_vec(pos), truth, k=k, R=k)
        out["refined_recall_at_%d" % k] = api.recall(to_vec(ri.cpu().numpy()), truth, k=k, R=k)
        out["exact_reranked_recall_at_%d" % k] = api.recall(fi.cpu().numpy(), truth, k=k, R=k)
        out["bytes_per_vector"] = dict(dtc_stream=len(payload) / n, plain_pq_code=8, refine_level=lvl.M2,
                                       dtc_plus_refine=len(payload) / n + lvl.M2, raw_fp32=4 * args.dim)
        lvl.close()
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
