#!/usr/bin/env python
"""Measurements of the candidate search on the bench-shaped vectors; prints one JSON line.

(a) The PQ top-`--cand` lists re-scored to top-`--topk` by candidate_search_torch, beside dpq_refine_rerank_device and
    dpq_flat_rerank_device on the SAME lists (the arrangements of scripts/dev_refine.py): synchronous calls, the three
    taking turns, the median of `--reps` rounds.
(b) `--nq` queries with `--long` random ids each, beside query_batch_filtered under ONE filter of the same selectivity.
(c) candidate_distances_torch on (a)'s lists.
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


def taking_turns(fns, reps):
    """{name: spread of ms per synchronous call}: one warm-up each, then `reps` rounds in which every call runs once."""
    import torch
    ms = {name: [] for name in fns}
    for name, fn in fns.items():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: spread(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--cand", type=int, default=1000)
    ap.add_argument("--long", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    n, k = args.n, args.topk
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, n_cand=args.cand, n_long=args.long, reps=args.reps)
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    with api.FlatIndex(base) as flat, api.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        flat.set_id_map(tree.vec_id)
        idx.set_codebook(cb)
        lvl = api.RefineLevel.build(idx, base, vec_id=tree.vec_id)
        pos, pos_d = idx.query_batch(qs, args.cand)
        d_q, d_c = torch.from_numpy(qs).cuda(), torch.from_numpy(pos).cuda()
        # (a) and (c): the same lists through the three rankers and the distance form
        res = {}
        turns = taking_turns({
            "candidate_search_device": lambda: res.__setitem__("cand", idx.candidate_search_torch(d_q, d_c, k)),
            "refine_rerank_device": lambda: lvl.rerank_torch(d_q, d_c, k),
            "flat_rerank_device": lambda: flat.rerank_torch(d_q, d_c, k),
            "candidate_distances_device": lambda: res.__setitem__("dist", idx.candidate_distances_torch(d_q, d_c)),
        }, args.reps)
        out["rescoring_top%d_to_top%d_call_ms" % (args.cand, k)] = turns
        ci, cd = res["cand"][0].cpu().numpy(), res["cand"][1].cpu().numpy()
        out["rescored_equals_pq_prefix"] = bool(np.array_equal(ci, pos[:, :k]) and
                                                np.array_equal(cd.view(np.uint32), pos_d[:, :k].view(np.uint32)))
        out["distances_equal_pq_distances"] = bool(np.array_equal(res["dist"].cpu().numpy().view(np.uint32), pos_d.view(np.uint32)))
        # (b): long random lists beside one filter of the same selectivity
        rng = np.random.default_rng(5)
        long_c = rng.integers(0, n - 1, size=(args.nq, args.long)).astype(np.int32)
        d_l = torch.from_numpy(long_c).cuda()
        mask = np.zeros(n + 1, dtype=bool)
        mask[rng.choice(n - 1, size=args.long, replace=False)] = True
        with api.IdFilter.from_mask(idx, mask) as f:
            turns = taking_turns({
                "candidate_search_device": lambda: idx.candidate_search_torch(d_q, d_l, k),
                "query_batch_device_filtered": lambda: idx.query_batch_filtered_torch(d_q, k, f),
            }, args.reps)
        out["random_%d_ids_per_query_call_ms" % args.long] = turns
        out["filter_selectivity"] = args.long / n
        lvl.close()
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
