#!/usr/bin/env python
"""Measurements of the IVF training on the bench-shaped vectors; prints one JSON line, asserts nothing.

Per nlist: train_ivf_centroids for `--iters` rounds beside the torch k-means of dev_ivf_search.py for the same rounds (the
calls taking turns, median [min - max] of `--reps` rounds), with the library's own phase times (assign / update / repair
from device events, the host round trips as rounds_ms - gpu_ms).  The assignment alone: ivf_assign_torch over the index's
million reconstructions beside the existing chain for the same rows -- IVF.build, which reconstructs, runs the exact
search at k = 1 and makes the lists -- and IVF.from_labels, which makes the lists alone.  Quality: recall@top_k of IVF.search against the exhaustive PQ answer
with library-trained and torch-trained centroids.  A `rocprofv3 --kernel-trace --stats` run of this script with
--trace-only gives the per-kernel split.
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
from dev_ivf_search import kmeans, nearest  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true", help="one training call and one assignment, for a kernel trace")
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    n, k = args.n, args.topk
    out = dict(n=n, dim=args.dim, iters=args.iters, reps=args.reps)
    d_base = torch.from_numpy(base).cuda()
    if args.trace_only:
        cents, st = api.train_ivf_centroids(base, args.nlist[0], max_iters=args.iters, seed=3)
        api.ivf_assign_torch(torch.from_numpy(cents).cuda(), d_base)
        torch.cuda.synchronize()
        print(json.dumps(dict(out, nlist=args.nlist[0], stats=st)))
        return

    trained = {}
    for nlist in args.nlist:
        stats = []

        def lib_train():
            c, st = api.train_ivf_centroids(base, nlist, max_iters=args.iters, seed=3)
            stats.append(st)
            return c

        ms = taking_turns({"train_ivf_centroids": lib_train, "torch_kmeans": lambda: kmeans(d_base, nlist, args.iters, 3)},
                          args.reps)
        med = lambda key: float(np.median([s[key] for s in stats[1:]]))
        st = stats[-1]
        out["nlist_%d" % nlist] = dict(
            call_ms=ms, iters_run=st["iters_run"], converged=st["converged"], reseeded=st["reseeded"],
            distortion_first=st["distortion"][0], distortion_last=st["distortion"][-1],
            phases_ms={key: med(key) for key in ("wall_ms", "rounds_ms", "gpu_ms", "assign_ms", "update_ms", "repair_ms")},
            host_round_trips_ms=med("rounds_ms") - med("gpu_ms"), syncs_per_round=1)
        trained[nlist] = (lib_train(), kmeans(d_base, nlist, args.iters, 3))

    # the assignment alone, and the existing chain, over the index's reconstructions
    nlist = args.nlist[0]
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    cb, _ = api.train_codebook(base, 8, 256, max_iters=25, seed=0)
    tree = api.DeltaTree(api.encode_pq(base, cb), codebook=cb, device=0)
    vec_id = torch.from_numpy(tree.vec_id.astype(np.int64)).cuda()
    with api.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        d_q = torch.from_numpy(qs).cuda()
        pq_ids = idx.query_batch_torch(d_q, k)[0].cpu().numpy()
        lib_c, torch_c = trained[nlist]
        d_cents = torch.from_numpy(lib_c).cuda()
        ids = torch.arange(n, dtype=torch.int32, device="cuda")
        if n % 2 == 0:
            ids[n - 1] = n
        recon = idx.reconstruct_torch(ids)
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        dists = torch.empty(n, dtype=torch.float32, device="cuda")

        def assign():
            api.ivf_assign_torch(d_cents, recon, out_labels=labels, out_dists=dists)

        def build():
            api.IVF.build(idx, lib_c).close()

        def from_labels():
            api.IVF.from_labels(idx, labels, nlist).close()

        assign()
        out["assignment"] = dict(nlist=nlist, call_ms=taking_turns(
            {"ivf_assign_device": assign, "ivf_build_existing_chain": build, "ivf_from_labels_lists_only": from_labels},
            args.reps))
        with api.IVF.build(idx, lib_c) as built, api.IVF.from_labels(idx, labels, nlist) as mine:
            out["assignment"]["same_lists_as_ivf_build"] = bool(all(np.array_equal(a, b)
                                                                    for a, b in zip(built.lists(), mine.lists())))
        # quality: lists by the original vectors, library-trained beside torch-trained centroids
        quality = {}
        for name, cents in (("library", lib_c), ("torch", torch_c.cpu().numpy())):
            if name == "library":
                vec_labels = api.ivf_assign_torch(torch.from_numpy(cents).cuda(), d_base)[0]
            else:
                vec_labels = nearest(d_base, torch_c).to(torch.int32)
            with api.IVF.from_labels(idx, vec_labels[vec_id].contiguous(), nlist, centroids=cents) as ivf:
                quality[name] = {"nprobe_%d" % p: api.recall(ivf.search_torch(d_q, p, k)[0].cpu().numpy(), pq_ids)
                                 for p in args.nprobe}
        out["recall_at_%d_vs_exhaustive_pq" % k] = quality
    tree.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
