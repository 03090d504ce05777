#!/usr/bin/env python
"""Measurements of the range search over the raw-vector IVF on the bench-shaped vectors; prints one JSON
line, writes it to --out, and asserts nothing.

Per format -- fp32, f16, u8 (the vectors mapped to bytes by one affine map of their whole range) and bits (one bit per
dimension against the per-dimension mean) -- one handle with 1024 lists from train_ivf_centroids over the fp32 vectors, and
three radii, the same for every query: the median over the queries of the distance to the 10th, 100th and 1000th exact
neighbour in the handle's own units ("r10", "r100", "r1000").  Per nprobe and radius, ms per synchronous host call, the calls
taking turns, median [min - max] of --reps rounds:
  range        range_search_probes over probe()'s lists (the whole call: both passes, the sort, the keys down and split);
  top100       search_probes top-100 over the same lists, in the same process;
and beside them, counted once:
  found / exhaustive   results per query of the range call and of the handle's exhaustive range_search at the radius;
  dropped_pairs        the share of (query, list) pairs without a hit, which the emit pass leaves before it reads their list.
Once per format and radius: flat_range, the exhaustive range_search, 3 rounds.  The count and the emit launch are not timed
on their own here: the library has no hook that runs one pass alone.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--formats", nargs="+", default=["f32", "f16", "u8", "bits"])
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_range_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    n, D, nlist = args.n, args.dim, args.nlist
    base = synth.make_clustered_vectors(n, D, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, D, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=n, dim=D, nq=args.nq, nlist=nlist, reps=args.reps, train_iters=args.train_iters)
    cents, _ = api.train_ivf_centroids(base, nlist, max_iters=args.train_iters)
    labels, _ = api.ivf_assign(cents, base)
    labels = labels.astype(np.int32)
    lo, hi = float(base.min()), float(base.max())
    scale = 255.0 / (hi - lo)
    as_bytes = lambda a: np.clip(np.rint((a - lo) * scale), 0, 255).astype(np.uint8)
    thr = base.mean(axis=0).astype(np.float32)
    with api.FlatIndex(base) as ref, api.FlatIVF.from_labels(ref, labels, nlist, centroids=cents) as coarse:
        probes = {p: coarse.probe(qs, p)[0] for p in args.nprobe}
    opened = {"f32": lambda: (api.FlatIndex(base), api.FlatIVF, qs),
              "f16": lambda: (api.FlatIndexHalf(base, "f16"), api.FlatIVF, qs),
              "u8": lambda: (api.FlatIndexU8(as_bytes(base)), api.FlatIVFBytes, as_bytes(qs)),
              "bits": lambda: (api.FlatIndexBits(api.bits_from_float(base, thr), D), api.FlatIVFBits, api.bits_from_float(qs, thr))}
    for fmt in args.formats:
        flat, cls, q = opened[fmt]()
        res = out[fmt] = {}
        with flat, cls.from_labels(flat, labels, nlist) as ivf:
            near = flat.search(q, 1000)[1]
            radii = {"r%d" % k: float(np.nextafter(np.float32(np.median(near[:, k - 1])), np.float32(np.inf))) for k in (10, 100, 1000)}
            res["radii"] = radii
            res["flat_range_ms"] = taking_turns({name: (lambda r=r: flat.range_search(q, r)) for name, r in radii.items()}, 3)
            whole = {name: flat.range_search(q, r)[0][-1] / len(q) for name, r in radii.items()}
            for p, lists in probes.items():
                at = res["nprobe_%d" % p] = {}
                fns = {"top100": lambda: ivf.search_probes(q, lists, 100)}
                for name, r in radii.items():
                    fns["range_" + name] = lambda r=r: ivf.range_search_probes(q, lists, r)
                    lims, ids, _ = fns["range_" + name]()
                    hit = len(np.unique(np.repeat(np.arange(len(q)), np.diff(lims)) * nlist + labels[ids]))
                    at[name] = dict(found=float(lims[-1]) / len(q), exhaustive=float(whole[name]),
                                    dropped_pairs=1.0 - hit / float((lists >= 0).sum()))
                at["call_ms"] = taking_turns(fns, args.reps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
