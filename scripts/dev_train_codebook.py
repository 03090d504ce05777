#!/usr/bin/env python
"""Measurements of the codebook trainer on the bench vectors; prints one JSON line.

  --mode kernels   `--reps` one-round trainings and `--reps` dpq_encode_pq calls on the same vectors and the same
                   codebook, so that a `rocprofv3 --kernel-trace --stats` run of this mode lists
                   train_assign_kernel and encode_pq_kernel side by side (kernel times come from that trace,
                   not from this process); checks that both give the same labels through the one-round update
  --mode run       `--reps` whole trainings of --iters rounds: wall and device time, the split per phase
  --mode quality   distortion on all vectors of the trained codebook against bench.py's stand-in
                   (synth.kmeans_codebook), both under the trainer's fp32 assignment, and the DTC payload bytes and
                   unique-code fraction of the two indexes
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltapq_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "run", "quality"), default="run")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(mode=args.mode, n=args.n, dim=args.dim, M=args.m, K=args.k)
    if args.mode == "kernels":
        start, _ = api.train_codebook(base, args.m, args.k, max_iters=1, seed=0)    # warm-up; a codebook to share
        for _ in range(args.reps):
            after, st = api.train_codebook(base, args.m, args.k, max_iters=1, init=start)
        for _ in range(args.reps):
            codes = api.encode_pq(base, start)
        # same labels: the one-round update of the trainer is the mean of the encoder's labels (integer-valued
        # vectors: exact in any order)
        Ds = start.shape[2]
        m = args.m - 1
        sub = base[:, m * Ds:(m + 1) * Ds].astype(np.float64)
        k = int(np.bincount(codes[:, m], minlength=args.k).argmax())
        want = (sub[codes[:, m] == k].sum(0) / (codes[:, m] == k).sum()).astype(np.float32)
        out.update(reps=args.reps, labels_agree=bool(np.array_equal(want, after[m, k])), assign_ms_events=st["assign_ms"])
    elif args.mode == "run":
        api.train_codebook(base, args.m, args.k, max_iters=1, seed=0)               # warm-up
        runs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            cb, st = api.train_codebook(base, args.m, args.k, max_iters=args.iters, seed=0)
            st["call_ms"] = (time.perf_counter() - t0) * 1e3
            runs.append(st)
        for key in ("call_ms", "wall_ms", "rounds_ms", "gpu_ms", "assign_ms", "update_ms", "repair_ms"):
            vals = [r[key] for r in runs]
            out[key] = dict(median=statistics.median(vals), min=min(vals), max=max(vals))
        last = runs[-1]
        out.update(reps=args.reps, iters_run=last["iters_run"], converged=last["converged"], reseeded=last["reseeded"],
                   distortion_first=last["distortion"][0], distortion_last=last["distortion"][-1],
                   host_round_trip_ms_per_round=(out["rounds_ms"]["median"] - out["gpu_ms"]["median"]) / last["iters_run"])
    else:
        trained, st = api.train_codebook(base, args.m, args.k, max_iters=args.iters, seed=0)
        standin = synth.kmeans_codebook(base, args.m, args.k, iters=6, seed=102)
        for name, cb in (("trained", trained), ("standin", standin)):
            _, ev = api.train_codebook(base, args.m, args.k, max_iters=1, init=cb)  # round 1's distortion is cb's
            codes = api.encode_pq(base, cb)
            uniq = len(np.unique(codes, axis=0)) / float(len(codes))
            tree = api.DeltaTree(codes, codebook=cb, device=0)
            out[name] = dict(distortion=ev["distortion"][0], payload_bytes=tree.stats["n_bytes"], n_diffs=tree.stats["n_diffs"],
                             unique_code_fraction=uniq)
            tree.close()
        out.update(iters_run=st["iters_run"], distortion_ratio=out["trained"]["distortion"] / out["standin"]["distortion"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
