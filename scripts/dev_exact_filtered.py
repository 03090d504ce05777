#!/usr/bin/env python
"""Measurements of the exact filtered search on the vectors of dev_exact_search.py; prints one JSON line.

  exact   `--reps` calls of FlatIndex.search and, per share of eligible rows (100 %, 10 %, 1 %, 0.1 %; drawn at random, and
          as one contiguous block), of FlatIdFilter creation and FlatIndex.search_filtered (host buffers in and out)
  pq      the chain a user runs (train, encode, DeltaTree), then DeltaPQIndex.query_batch_filtered under the same random
          bitmaps translated with bitmap_to_dfs: its time and its recall@topk against the exact filtered answer
`--kind u8` runs the exact part on a byte handle (the vectors rounded to bytes).
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

SHARES = (1.0, 0.1, 0.01, 0.001)


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
    ap.add_argument("--mode", choices=("exact", "all"), default="all")
    ap.add_argument("--kind", choices=("fp32", "u8"), default="fp32")
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
    if args.kind == "u8":
        lo, hi = float(base.min()), float(base.max())
        base = np.clip(np.rint((base - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
        qs = np.clip(np.rint((qs - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    n, k = args.n, args.topk
    rng = np.random.default_rng(102)
    masks = {}
    for s in SHARES:
        m = int(round(n * s))
        rnd = np.zeros(n, dtype=bool)
        rnd[rng.choice(n, size=m, replace=False)] = True
        blk = np.zeros(n, dtype=bool)
        b0 = (n - m) // 2
        blk[b0:b0 + m] = True
        masks[s] = dict(random=rnd, block=blk)
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, reps=args.reps, kind=args.kind, shares={})
    truth = {}
    with (api.FlatIndex if args.kind == "fp32" else api.FlatIndexU8)(base) as flat:
        (ui, ud), out["search_call_ms"] = timed(lambda: flat.search(qs, k), args.reps)
        for s in SHARES:
            row = {}
            for shape in ("random", "block"):
                words, n_bits = api.IdFilter.pack_mask(masks[s][shape])
                made = []
                (_, row[shape + "_filter_create_ms"]) = timed(lambda: made.append(api.FlatIdFilter(flat, words, n_bits)) or
                                                              made.pop().close(), args.reps)
                with api.FlatIdFilter(flat, words, n_bits) as ff:
                    row["eligible"] = ff.n_allowed
                    (fi, fd), row[shape + "_search_filtered_call_ms"] = timed(lambda: flat.search_filtered(qs, k, ff), args.reps)
                if shape == "random":
                    truth[s] = fi
                if s == 1.0:
                    row[shape + "_equals_unfiltered"] = bool(fi.tobytes() == ui.tobytes() and fd.tobytes() == ud.tobytes())
            out["shares"]["%g" % s] = row
    if args.mode == "all" and args.kind == "fp32":
        cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
        codes = api.encode_pq(base, cb)
        tree = api.DeltaTree(codes, codebook=cb, device=0)
        with api.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0) as idx:
            idx.set_codebook(cb)
            (_, out["pq_query_batch_call_ms"]) = timed(lambda: idx.query_batch(qs, k), args.reps)
            for s in SHARES:
                words, n_bits = api.IdFilter.pack_mask(masks[s]["random"])
                with api.IdFilter(idx, *api.bitmap_to_dfs(words, n_bits, tree.vec_id)) as filt:
                    (pos, _), ms = timed(lambda: idx.query_batch_filtered(qs, k, filt), args.reps)
                p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
                found = np.where(pos < 0, -1, tree.vec_id[np.clip(p, 0, n - 1)].astype(np.int64)).astype(np.int32)
                row = out["shares"]["%g" % s]
                row["pq_query_batch_filtered_call_ms"] = ms
                row["pq_filtered_recall_at_%d" % k] = api.recall(found, truth[s], k=k, R=k)
        tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
