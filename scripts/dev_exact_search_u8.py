#!/usr/bin/env python
"""Measurements of the exact search over byte vectors against the fp32 exact search of the same data,
both in one run; prints one JSON line and writes it to profiles/exact_search_u8_line.json.

The vectors are the bench vectors of scripts/dev_exact_search.py quantised to bytes: np.clip(np.rint(a * x + b), 0, 255)
with the affine map a = 1, b = 0 -- make_clustered_vectors already gives integers in 0..218, so the bytes are the values.

  search   `--reps` exact top-`--topk` searches of `--nq` queries over all `--n` vectors after a warm-up call:
           FlatIndexU8.search on the bytes, FlatIndex.search on the same data widened to fp32 (host buffers in and out)
  rerank   exact re-rank of `--rerank` candidates per query to top-`--topk`, host buffers and device tensors, on both
           handles; the candidates are the exact top-`--rerank` ids in a shuffled order (no PQ index is built here)
Every pair of answers is asserted equal bit for bit.  A `rocprofv3 --kernel-trace --stats` run of this script gives the
per-kernel split (flat_dist_u8_kernel against flat_dist_kernel on the same stripes).
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


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def quantise(x):
    return np.clip(np.rint(1.0 * x + 0.0), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("search", "all"), default="all")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rerank", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_search_u8_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    base8 = quantise(synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7))
    qs8 = quantise(synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7))
    base32, qs32 = base8.astype(np.float32), qs8.astype(np.float32)
    out = dict(n=args.n, dim=args.dim, nq=args.nq, top_k=args.topk, reps=args.reps, affine_map=[1.0, 0.0])
    with api.FlatIndexU8(base8) as f8, api.FlatIndex(base32) as f32:
        a8, out["u8_search_call_ms"] = timed(lambda: f8.search(qs8, args.topk), args.reps)
        a32, out["fp32_search_call_ms"] = timed(lambda: f32.search(qs32, args.topk), args.reps)
        assert same(a8, a32), "the byte search and the fp32 search differ"
        out["search_bits_equal"] = True
        out["search_fp32_over_u8"] = out["fp32_search_call_ms"]["median"] / out["u8_search_call_ms"]["median"]
        if args.mode == "all":
            import torch
            cand, _ = f8.search(qs8, args.rerank)
            cand = np.ascontiguousarray(np.random.default_rng(5).permuted(cand, axis=1))
            r8, out["u8_rerank_call_ms"] = timed(lambda: f8.rerank(qs8, cand, args.topk), args.reps)
            r32, out["fp32_rerank_call_ms"] = timed(lambda: f32.rerank(qs32, cand, args.topk), args.reps)
            assert same(r8, r32) and same(r8, a8), "the re-ranked answers differ"
            d_c, d_q8, d_q32 = torch.from_numpy(cand).cuda(), torch.from_numpy(qs8).cuda(), torch.from_numpy(qs32).cuda()

            def on_device(f, q):
                r = f.rerank_torch(q, d_c, args.topk)
                torch.cuda.synchronize()
                return r
            t8, out["u8_rerank_device_call_ms"] = timed(lambda: on_device(f8, d_q8), args.reps)
            t32, out["fp32_rerank_device_call_ms"] = timed(lambda: on_device(f32, d_q32), args.reps)
            assert same((t8[0].cpu().numpy(), t8[1].cpu().numpy()), r8) and same((t32[0].cpu().numpy(), t32[1].cpu().numpy()), r8)
            out["rerank_bits_equal"] = True
            out["rerank_device_fp32_over_u8"] = (out["fp32_rerank_device_call_ms"]["median"] /
                                                 out["u8_rerank_device_call_ms"]["median"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
