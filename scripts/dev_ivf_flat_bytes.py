#!/usr/bin/env python
"""Measurements of the IVF search over byte vectors on the bench-shaped vectors taken as bytes; prints
one JSON line, writes it to --out, and asserts nothing.

The bench vectors are mapped to uint8 by one affine map of their whole range.  One FlatIndexU8 over them and one FlatIndex
over the same bytes widened to fp32; 1024 lists from train_ivf_centroids over the widened vectors, the same centroids for
FlatIVFBytes.build and FlatIVF.build.  Per nprobe:
  recall   recall@top_k of FlatIVFBytes.search_torch against the exhaustive FlatIndexU8.search;
  call_ms  ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds: the byte search_torch at
           the group G = 4, 8, 16 (DPQ_FLAT_IVF_GROUP, read per call under DPQ_DEV=1), the fp32 FlatIVF.search_torch over
           the widened vectors at its shipped group, and the byte index's exhaustive host call FlatIndexU8.search.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_bytes_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, k, nlist = args.n, args.topk, args.nlist
    base = synth.make_clustered_vectors(n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    lo, hi = float(base.min()), float(base.max())
    as_bytes = lambda a: np.clip(np.rint((a - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    base8, qs8 = as_bytes(base), as_bytes(qs)
    wide, wq = base8.astype(np.float32), qs8.astype(np.float32)
    del base, qs
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters)
    cents, _ = api.train_ivf_centroids(wide, nlist, max_iters=args.train_iters)
    d_q8, d_wq = torch.from_numpy(qs8).cuda(), torch.from_numpy(wq).cuda()
    with api.FlatIndexU8(base8) as flat8, api.FlatIVFBytes.build(flat8, cents) as ivf8, \
            api.FlatIndex(wide) as flat32, api.FlatIVF.build(flat32, cents) as ivf32:
        truth = flat8.search(qs8, k)[0]
        out["lists"] = ivf8.info()
        out["same_lists_as_fp32"] = bool(all(np.array_equal(a, b) for a, b in zip(ivf8.lists(), ivf32.lists())))

        def at(G, nprobe):
            def call():
                os.environ["DPQ_FLAT_IVF_GROUP"] = str(G)
                return ivf8.search_torch(d_q8, nprobe, k)
            return call

        def fp32(nprobe):
            def call():
                os.environ.pop("DPQ_FLAT_IVF_GROUP", None)
                return ivf32.search_torch(d_wq, nprobe, k)
            return call

        for nprobe in args.nprobe:
            fns = {"bytes_search_torch_G%d" % G: at(G, nprobe) for G in (4, 8, 16)}
            fns["fp32_search_torch"] = fp32(nprobe)
            fns["bytes_flat_search_host"] = lambda: flat8.search(qs8, k)
            answers = {name: [a.cpu().numpy() for a in fns[name]()] for name in fns if name.endswith(("G4", "G8", "G16", "torch"))}
            ref = answers["bytes_search_torch_G4"]
            out["nprobe_%d" % nprobe] = dict(
                recall=api.recall(ref[0], truth),
                same_answer_for_every_G=bool(all(np.array_equal(ref[0], answers["bytes_search_torch_G%d" % G][0]) for G in (8, 16))),
                same_answer_as_fp32=bool(np.array_equal(ref[0], answers["fp32_search_torch"][0]) and
                                         np.array_equal(ref[1].view(np.uint32), answers["fp32_search_torch"][1].view(np.uint32))),
                call_ms=taking_turns(fns, args.reps))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
