#!/usr/bin/env python
"""Measurements of the IVF search over raw vectors on the bench-shaped vectors; prints one JSON line,
writes it to --out, and asserts nothing.

One FlatIndex over the vectors, 1024 lists from train_ivf_centroids (FlatIVF.build).  Per nprobe:
  rows_per_query  the mean number of rows in the union of a query's probed lists;
  recall          recall@top_k of FlatIVF.search against the exhaustive FlatIndex.search;
  call_ms         ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds:
                  search_torch at the group G = 4, 8, 16 (DPQ_FLAT_IVF_GROUP, read per call under DPQ_DEV=1), the host
                  form FlatIVF.search (the shipped G) beside the exhaustive host call FlatIndex.search (the exhaustive search
                  has no device-tensor form), and, where every query's probed ids fit 16384, rerank_torch over those ids.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["DPQ_DEV"] = "1"  # the group knob is a developer switch
from deltapq_amd import api, synth  # noqa: E402
from dev_candidate_search import taking_turns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, k, nlist = args.n, args.topk, args.nlist
    base = synth.make_clustered_vectors(n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters)
    cents, _ = api.train_ivf_centroids(base, nlist, max_iters=args.train_iters)
    d_q = torch.from_numpy(qs).cuda()
    with api.FlatIndex(base) as flat, api.FlatIVF.build(flat, cents) as ivf:
        truth = flat.search(qs, k)[0]
        out["lists"] = ivf.info()
        offsets, ids = ivf.lists()

        def at(G, nprobe):
            def call():
                os.environ["DPQ_FLAT_IVF_GROUP"] = str(G)
                return ivf.search_torch(d_q, nprobe, k)
            return call

        def host(nprobe):
            def call():
                os.environ.pop("DPQ_FLAT_IVF_GROUP", None)
                return ivf.search(qs, nprobe, k)
            return call

        for nprobe in args.nprobe:
            probed, _ = ivf.probe(qs, nprobe)
            cand = [np.concatenate([ids[offsets[l]:offsets[l + 1]] for l in row]) for row in probed]
            longest = max(len(c) for c in cand)
            fns = {"search_torch_G%d" % G: at(G, nprobe) for G in (4, 8, 16)}
            fns["search_host"] = host(nprobe)
            fns["flat_search_host"] = lambda: flat.search(qs, k)
            if longest <= 16384:
                padded = np.full((args.nq, longest), -1, dtype=np.int32)
                for i, c in enumerate(cand):
                    padded[i, :len(c)] = c
                d_cand = torch.from_numpy(padded).cuda()
                fns["rerank_torch_same_ids"] = lambda: flat.rerank_torch(d_q, d_cand, k)
            answers = {name: fns[name]()[0].cpu().numpy() for name in fns if name.startswith("search_torch")}
            out["nprobe_%d" % nprobe] = dict(
                rows_per_query=float(np.mean([len(c) for c in cand])), longest_union=int(longest),
                recall=api.recall(answers["search_torch_G16"], truth),
                same_answer_for_every_G=bool(np.array_equal(answers["search_torch_G4"], answers["search_torch_G8"]) and
                                             np.array_equal(answers["search_torch_G4"], answers["search_torch_G16"])),
                call_ms=taking_turns(fns, args.reps))
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
