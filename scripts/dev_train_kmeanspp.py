#!/usr/bin/env python
"""Measurements of the k-means++ start and the restarts of the codebook trainer on the bench
vectors; prints one JSON line and, with --out, writes it to a file (profiles/train_kmeanspp_line.json).

Un-profiled runs, one warm-up call first, medians with min and max over --reps calls:
  seeding    dpq_kmeanspp_seed alone, whole call (upload and split of the vectors included), at K and at K = 2:
             the difference is the K - 2 further steps
  runs       whole trainings of --iters rounds from the rows start, the k-means++ start, and k-means++ with three restarts
  quality    potential (dpq_train_potential) and distortion of the rows and the k-means++ codebooks, potential of the
             k-means++ start before any round, DTC payload bytes and diffs of the two indexes
No threshold: the comparison is against the rows start of the same session, whatever it shows.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltapq_amd import api, synth  # noqa: E402


def spread(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def timed(fn, reps):
    ms, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-index", action="store_true", help="skip the DTC payload of the two codebooks")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    M, K = args.m, args.k
    out = dict(n=args.n, dim=args.dim, M=M, K=K, iters=args.iters, reps=args.reps)
    api.train_codebook(base, M, K, max_iters=1, seed=0)                                   # warm-up
    api.kmeanspp_seed(base, M, 2, seed=0)

    out["seed_call_ms"], (seeded, seed_pot) = timed(lambda: api.kmeanspp_seed(base, M, K, seed=0), args.reps)
    out["seed_call_k2_ms"], _ = timed(lambda: api.kmeanspp_seed(base, M, 2, seed=0), args.reps)
    out["seed_steps_ms"] = out["seed_call_ms"]["median"] - out["seed_call_k2_ms"]["median"]
    out["seed_potential"] = float(seed_pot.sum())

    results = {}
    for name, kw in (("rows", dict(start="rows")), ("pp", dict(start="kmeans++")),
                     ("pp_restarts3", dict(start="kmeans++", restarts=3))):
        call, (cb, st) = timed(lambda: api.train_codebook(base, M, K, max_iters=args.iters, seed=0, **kw), args.reps)
        results[name] = cb
        out[name] = dict(call_ms=call, wall_ms=st["wall_ms"], gpu_ms=st["gpu_ms"], assign_ms=st["assign_ms"],
                         update_ms=st["update_ms"], repair_ms=st["repair_ms"], iters_run=st["iters_run"],
                         converged=st["converged"], reseeded=st["reseeded"], distortion_first=st["distortion"][0],
                         distortion_last=st["distortion"][-1])
    for name, cb in results.items():
        out[name]["potential"] = float(api.train_potential(base, cb).sum())
        _, ev = api.train_codebook(base, M, K, max_iters=1, init=cb)                      # round 1's distortion is cb's
        out[name]["distortion"] = ev["distortion"][0]
        if name != "pp_restarts3" and not args.no_index:
            codes = api.encode_pq(base, cb)
            tree = api.DeltaTree(codes, codebook=cb, device=0)
            out[name].update(payload_bytes=tree.stats["n_bytes"], n_diffs=tree.stats["n_diffs"])
            tree.close()
    for name in ("pp", "pp_restarts3"):
        out[name]["potential_ratio_to_rows"] = out[name]["potential"] / out["rows"]["potential"]
        out[name]["call_ms_ratio_to_rows"] = out[name]["call_ms"]["median"] / out["rows"]["call_ms"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
