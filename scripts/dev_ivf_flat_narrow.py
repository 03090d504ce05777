#!/usr/bin/env python
"""Measurements of the IVF search over half-precision and scalar-quantised vectors on the bench-shaped
vectors; prints one JSON line, writes it to --out, and asserts nothing.

The bench vectors are stored as f16, bf16, sq8 and sq4 (the last two under sq_train of the base).  1024 lists from
train_ivf_centroids over the fp32 base, labels from ivf_assign over it: the same lists for every structure.  Per format,
one narrow handle and one fp32 FlatIndex over the same rows widened or decoded, a FlatIVF on each.  Per nprobe:
  recall   recall@top_k of the narrow FlatIVF.search_torch against the exhaustive fp32 FlatIndex.search of the base;
  call_ms  ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds: the narrow search_torch
           at the group G = 4, 8, 16 (DPQ_FLAT_IVF_GROUP, read per call under DPQ_DEV=1), the fp32 FlatIVF.search_torch
           over the widened rows at its shipped group (the baseline), and the narrow handle's exhaustive host call.
row_bytes: the device bytes of a handle's rows, n times the padded row of its format (computed from the storage rule).
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

FORMATS = ("f16", "bf16", "sq8", "sq4")


def stored(base, fmt):
    """(opens the narrow handle, the fp32 rows it stands for, bytes of a stored row)."""
    D = base.shape[1]
    if fmt in api.HALF_FORMATS:
        bits16 = api.half_from_float(base, fmt)
        return (lambda: api.FlatIndexHalf(bits16, fmt)), api.half_to_float(bits16, fmt), 2 * ((D + 7) & ~7)
    bits = 8 if fmt == "sq8" else 4
    lo, step = api.sq_train(base, bits)
    codes = api.sq_encode(base, lo, step, bits)
    row = (D + 15) & ~15 if bits == 8 else ((D + 31) & ~31) // 2
    return (lambda: api.FlatIndexSQ(codes, lo, step, bits)), api.sq_decode(codes, lo, step, bits), row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--formats", nargs="+", default=list(FORMATS))
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_narrow_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, k, nlist = args.n, args.topk, args.nlist
    base = synth.make_clustered_vectors(n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters,
               row_bytes=dict(fp32=n * 4 * ((args.dim + 3) & ~3)))
    cents, _ = api.train_ivf_centroids(base, nlist, max_iters=args.train_iters)
    labels, _ = api.ivf_assign(cents, base)
    with api.FlatIndex(base) as exact:
        truth = exact.search(qs, k)[0]
    d_q = torch.from_numpy(qs).cuda()
    for fmt in args.formats:
        opener, wide, row = stored(base, fmt)
        out["row_bytes"][fmt] = n * row
        with opener() as flat, api.FlatIVF.from_labels(flat, labels, nlist, centroids=cents) as ivf, \
                api.FlatIndex(wide) as flat32, api.FlatIVF.from_labels(flat32, labels, nlist, centroids=cents) as ivf32:
            del wide
            res = out[fmt] = dict(lists=ivf.info())

            def at(G, nprobe):
                def call():
                    os.environ["DPQ_FLAT_IVF_GROUP"] = str(G)
                    return ivf.search_torch(d_q, nprobe, k)
                return call

            def fp32(nprobe):
                def call():
                    os.environ.pop("DPQ_FLAT_IVF_GROUP", None)
                    return ivf32.search_torch(d_q, nprobe, k)
                return call

            for nprobe in args.nprobe:
                fns = {"narrow_search_torch_G%d" % G: at(G, nprobe) for G in (4, 8, 16)}
                fns["fp32_search_torch"] = fp32(nprobe)
                answers = {name: [a.cpu().numpy() for a in fn()] for name, fn in fns.items()}
                fns["narrow_flat_search_host"] = lambda: flat.search(qs, k)
                ref = answers["narrow_search_torch_G4"]
                res["nprobe_%d" % nprobe] = dict(
                    recall=api.recall(ref[0], truth),
                    same_answer_as_fp32_and_for_every_G=bool(all(
                        np.array_equal(ref[0], a[0]) and np.array_equal(ref[1].view(np.uint32), a[1].view(np.uint32))
                        for a in answers.values())),
                    call_ms=taking_turns(fns, args.reps))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
