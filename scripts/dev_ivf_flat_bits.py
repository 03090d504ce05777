#!/usr/bin/env python
"""Measurements of the IVF search over binary vectors on bench-shaped vectors of --dim dimensions
binarised to one bit each; prints one JSON line, writes it to --out, and asserts nothing.

The vectors are made and binarised a chunk at a time (bits_from_float against per-dimension thresholds, the means of the
first chunk), so that a million rows of 1024 dimensions never stand in host memory as floats.  1024 lists: the centroids
are train_ivf_centroids' over the first chunk's floats, binarised with the same thresholds (FlatIVFBits.build).  One
FlatIndexU8 over the same packed rows taken as bytes, with the same lists (FlatIVFBytes.from_labels), stands for the byte
scan over rows of the same length.  Per nprobe:
  recall   recall@top_k of FlatIVFBits.search_torch against the exhaustive FlatIndexBits.search;
  call_ms  ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds: the binary search_torch at
           the group G = 4, 8, 16 (DPQ_FLAT_IVF_GROUP, read per call under DPQ_DEV=1), the byte
           FlatIVFBytes.search_probes_torch over the same rows and the same probes at its shipped group, and the binary
           index's exhaustive host call FlatIndexBits.search.
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
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_bits_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, D, k, nlist = args.n, args.dim, args.topk, args.nlist
    make = lambda rows, seed: synth.make_clustered_vectors(rows, D, seed=seed, n_clusters=20000, spread=12.0, centre_seed=7)
    first = make(min(args.chunk, n), 100)
    thr = first.mean(axis=0).astype(np.float32)
    cents = api.bits_from_float(api.train_ivf_centroids(first, nlist, max_iters=args.train_iters)[0], thr)
    parts = [api.bits_from_float(first, thr)]
    del first
    for i, r0 in enumerate(range(args.chunk, n, args.chunk)):
        parts.append(api.bits_from_float(make(min(args.chunk, n - r0), 200 + i), thr))
    bits = np.concatenate(parts)
    del parts
    qs = api.bits_from_float(make(args.nq, 101), thr)
    out = dict(n=n, dim=D, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters)
    d_q = torch.from_numpy(qs).cuda()
    with api.FlatIndexBits(bits, D) as flat, api.FlatIVFBits.build(flat, cents) as ivf, api.FlatIndexU8(bits) as flat8:
        truth = flat.search(qs, k)[0]
        out["lists"] = ivf.info()
        offsets, ids = ivf.lists()
        labels = np.full(n, -1, dtype=np.int32)
        labels[ids] = np.repeat(np.arange(nlist, dtype=np.int32), np.diff(offsets))
        with api.FlatIVFBytes.from_labels(flat8, labels, nlist) as ivf8:

            def at(G, nprobe):
                def call():
                    os.environ["DPQ_FLAT_IVF_GROUP"] = str(G)
                    return ivf.search_torch(d_q, nprobe, k)
                return call

            def as_bytes(d_probes):
                def call():
                    os.environ.pop("DPQ_FLAT_IVF_GROUP", None)
                    return ivf8.search_probes_torch(d_q, d_probes, k)
                return call

            for nprobe in args.nprobe:
                d_probes = torch.from_numpy(ivf.probe(qs, nprobe)[0]).cuda()
                fns = {"bits_search_torch_G%d" % G: at(G, nprobe) for G in (4, 8, 16)}
                answers = {name: [a.cpu().numpy() for a in fn()] for name, fn in fns.items()}
                fns["bytes_search_probes_torch"] = as_bytes(d_probes)
                fns["bits_flat_search_host"] = lambda: flat.search(qs, k)
                ref = answers["bits_search_torch_G4"]
                out["nprobe_%d" % nprobe] = dict(
                    recall=api.recall(ref[0], truth),
                    same_answer_for_every_G=bool(all(np.array_equal(ref[0], answers["bits_search_torch_G%d" % G][0]) and
                                                     np.array_equal(ref[1], answers["bits_search_torch_G%d" % G][1])
                                                     for G in (8, 16))),
                    call_ms=taking_turns(fns, args.reps))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
