#!/usr/bin/env python
"""Measurements of the exact inner-product search on the bench-shaped vectors; prints one JSON line
and writes it to `--out`.

  search   `--reps` exact top-`--topk` searches of `--nq` queries over all `--n` vectors by inner product
           (dpq_flat_search_ip) and by L2 (dpq_flat_search) on the same handle, one after the other in each of `--rounds`
           rounds; the ratio of the two medians; the numpy restatement on `--cpu-queries` queries
  rerank   the index of DESIGN.md 5.14 (synth.kmeans_codebook, six rounds), its PQ inner-product top-`--rerank`
           (dpq_query_batch_ip), the exact re-rank of that answer to top-`--topk` on device tensors
           (dpq_flat_rerank_ip_device) and on host buffers; recall@topk of the PQ answer and of the re-ranked answer
           against the exact inner-product search
Every timing is `--reps` calls after a warm-up call, median and min - max on the host clock around the call.
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
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("search", "all"), default="all")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rerank", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--cpu-queries", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_ip_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=1, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=args.n, dim=args.dim, nq=args.nq, top_k=args.topk, reps=args.reps, rounds=args.rounds)
    with api.FlatIndex(base) as flat:
        ip_ms, l2_ms = [], []
        for _ in range(args.rounds):
            (truth, truth_s), ms = timed(lambda: flat.search_ip(qs, args.topk), args.reps)
            ip_ms += ms
            _, ms = timed(lambda: flat.search(qs, args.topk), args.reps)
            l2_ms += ms
        out["search_ip_call_ms"], out["search_l2_call_ms"] = spread(ip_ms), spread(l2_ms)
        out["search_ip_over_l2"] = out["search_ip_call_ms"]["median"] / out["search_l2_call_ms"]["median"]
        out["search_ip_triples_per_s"] = float(args.n) * args.nq * args.dim / (out["search_ip_call_ms"]["median"] * 1e-3)
        if args.cpu_queries > 0:
            import _exact_ip_restatement as X
            ci, cs = X.search(base, qs[:args.cpu_queries], args.topk)
            out["restatement_agrees"] = bool(np.array_equal(ci, truth[:args.cpu_queries]) and
                                             np.array_equal(cs.view(np.uint32), truth_s[:args.cpu_queries].view(np.uint32)))
        if args.mode == "all":
            import torch
            cb = synth.kmeans_codebook(base, 8, 256, iters=6, seed=102)
            codes = api.encode_pq(base, cb, device=0)
            tree = api.DeltaTree(codes, codebook=cb, device=0)
            flat.set_id_map(tree.vec_id)
            with api.DeltaPQIndex.open_memory(tree.payload(), args.n, 8, 256, device=0) as idx:
                idx.set_codebook(cb)
                res, ms = timed(lambda: idx.query_batch_ip(qs, args.rerank), args.reps)
                out["pq_ip_top%d_call_ms" % args.rerank] = spread(ms)
                pos = res[0]
            (ri, rs), ms = timed(lambda: flat.rerank_ip(qs, pos, args.topk), args.reps)
            out["rerank_ip_call_ms"] = spread(ms)
            d_q, d_c = torch.from_numpy(qs).cuda(), torch.from_numpy(pos).cuda()

            def on_device():
                r = flat.rerank_ip_torch(d_q, d_c, args.topk)
                torch.cuda.synchronize()
                return r
            (ti, ts), ms = timed(on_device, args.reps)
            out["rerank_ip_device_call_ms"] = spread(ms)
            out["rerank_variants_agree"] = bool(np.array_equal(ti.cpu().numpy(), ri) and
                                                np.array_equal(ts.cpu().numpy().view(np.uint32), rs.view(np.uint32)))
            n = args.n
            p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
            found = np.where(p >= 0, tree.vec_id[np.maximum(p, 0)].astype(np.int64), -1).astype(np.int32)
            out["pq_ip_recall_at_%d" % args.topk] = api.recall(found, truth, k=args.topk, R=args.topk)
            out["reranked_ip_recall_at_%d" % args.topk] = api.recall(ri, truth, k=args.topk, R=args.topk)
            out["pq_ip_recall_1_at_%d" % args.rerank] = api.recall(found, truth, k=1, R=args.rerank)
            tree.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
