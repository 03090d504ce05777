#!/usr/bin/env python
"""Measurements of the IVF search on the bench-shaped vectors; prints one JSON line.

nlist centroids from a torch k-means over the base.  Two structures over one index: lists by the nearest centroid of
every node's RECONSTRUCTION (IVF.build), and lists by the nearest centroid of its ORIGINAL vector, through vec_id
(IVF.from_labels with the centroids attached).  Per nprobe: ms per synchronous call of search_torch beside
query_batch_torch on the same handle and, where the probed lists fit 16384 ids per query, candidate_search_torch over the
same ids (the calls taking turns, median [min - max] of `--reps` rounds); codes scanned per query; recall@top_k against
the exhaustive PQ answer and against the exact ground truth.  A `rocprofv3 --kernel-trace --stats` run of this script gives
the per-kernel split.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deltapq_amd import api, synth  # noqa: E402
from dev_candidate_search import taking_turns  # noqa: E402


def nearest(x, cents, chunk=65536):
    """int64 [n]: the nearest centroid of every row of x (torch, fp32; measurement only, not the library's arithmetic)."""
    import torch
    c2 = (cents * cents).sum(1)
    out = []
    for i in range(0, x.shape[0], chunk):
        b = x[i:i + chunk]
        out.append(torch.argmin(c2[None, :] - 2.0 * (b @ cents.T), dim=1))
    return torch.cat(out)


def kmeans(x, nlist, iters, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    cents = x[torch.randperm(x.shape[0], generator=g)[:nlist].to(x.device)].clone()
    for _ in range(iters):
        lab = nearest(x, cents)
        sums = torch.zeros_like(cents).index_add_(0, lab, x)
        cnt = torch.bincount(lab, minlength=nlist).to(x.dtype)
        cents = torch.where(cnt[:, None] > 0, sums / cnt.clamp(min=1)[:, None], cents)
    return cents


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--kmeans-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    n, k, nlist = args.n, args.topk, args.nlist
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, kmeans_iters=args.kmeans_iters)
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    d_base = torch.from_numpy(base).cuda()
    cents_t = kmeans(d_base, nlist, args.kmeans_iters, 3)
    cents = cents_t.cpu().numpy()
    vec_labels = nearest(d_base, cents_t).to(torch.int32)
    labels = vec_labels[torch.from_numpy(tree.vec_id.astype(np.int64)).cuda()].contiguous()   # by DFS position
    del d_base
    with api.FlatIndex(base) as flat:
        truth = flat.search(qs, k)[0]                                          # vector ids
    with api.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        d_q = torch.from_numpy(qs).cuda()
        pq_ids = idx.query_batch_torch(d_q, k)[0].cpu().numpy()

        def vec_ids(pos):
            p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
            return np.where(p >= 0, tree.vec_id[np.clip(p, 0, n - 1)].astype(np.int64), -1).astype(np.int32)

        out["exhaustive_recall_vs_exact"] = api.recall(vec_ids(pq_ids), truth)
        by_recon, ms = timed(lambda: api.IVF.build(idx, cents))
        out["build_by_reconstruction_ms"] = ms
        by_vec, ms = timed(lambda: api.IVF.from_labels(idx, labels, nlist, centroids=cents))
        out["build_from_labels_ms"] = ms
        for name, ivf in (("by_reconstruction", by_recon), ("by_original_vector", by_vec)):
            inf = ivf.info()
            offsets, ids = ivf.lists()
            lens = np.diff(offsets)
            rows = {}
            for nprobe in args.nprobe:
                probes = ivf.probe(qs, nprobe)[0]
                scanned = lens[probes].sum(axis=1)
                fns = {"ivf_search_device": lambda: ivf.search_torch(d_q, nprobe, k),
                       "query_batch_device": lambda: idx.query_batch_torch(d_q, k)}
                if scanned.max() <= 16384:
                    cand = np.full((args.nq, int(scanned.max())), -1, dtype=np.int32)
                    for q in range(args.nq):
                        u = np.concatenate([ids[offsets[p]:offsets[p + 1]] for p in probes[q]])
                        cand[q, :len(u)] = u
                    d_c = torch.from_numpy(cand).cuda()
                    fns["candidate_search_device"] = lambda: idx.candidate_search_torch(d_q, d_c, k)
                got = ivf.search_torch(d_q, nprobe, k)[0].cpu().numpy()
                row = dict(call_ms=taking_turns(fns, args.reps), codes_scanned_per_query=float(scanned.mean()),
                           recall_vs_exhaustive_pq=api.recall(got, pq_ids), recall_vs_exact=api.recall(vec_ids(got), truth))
                if "candidate_search_device" in fns:
                    ci = idx.candidate_search_torch(d_q, d_c, k)[0].cpu().numpy()
                    row["equals_candidate_search"] = bool(np.array_equal(ci, got))
                rows["nprobe_%d" % nprobe] = row
            out[name] = dict(info=inf, **rows)
        by_recon.close()
        by_vec.close()
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
