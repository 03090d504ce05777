#!/usr/bin/env python
"""Measurements of the IVF search over raw vectors by inner product and under an id filter on the
bench-shaped vectors; prints one JSON line, writes it to --out, and asserts nothing.

Inner product ("ip" in the line): per format -- fp32, f16, sq8, u8 (the vectors mapped to bytes by one affine map of their
whole range) and i8 (those bytes lowered by 128) -- one handle with the lists and the centroids below (in the handle's units),
and per nprobe, ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds: search_ip_torch beside
search_torch (L2) of the same handle -- which probe different lists, by score and by distance -- and search_probes_ip_torch
beside search_probes_torch over the L2 probes, the same rows under both metrics; once per format the handle's exhaustive host
call search_ip.

Filters:

Per kind of rows -- fp32 (FlatIndex), u8 (the vectors mapped to bytes by one affine map of their whole range) and bits
(one bit per dimension against the per-dimension mean) -- one handle, 1024 lists from train_ivf_centroids over the fp32
vectors (the bits structure takes the fp32 structure's labels), and three filters that allow a random 100 %, 10 % and 0.1 %
of the rows.  Per nprobe and filter, ms per synchronous call, the calls taking turns, median [min - max] of --reps rounds:
  unfiltered       search_probes_torch without a filter;
  filtered_<pct>   search_probes_torch under the filter (the same probes: the coarse step does not see a filter);
and once per kind and filter, beside them:
  flat_filtered_<pct>  the handle's exhaustive host call search_filtered under the same filter (it has no device form).
same_as_cut_lists: whether the all-eligible answer equals the unfiltered one bit for bit.
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

SHARES = (("100", 1.0), ("10", 0.1), ("0.1", 0.001))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--kinds", nargs="+", default=["f32", "u8", "bits"], help="kinds of rows the filters are timed on")
    ap.add_argument("--ip-formats", nargs="+", default=["f32", "f16", "sq8", "u8", "i8"])
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_flat_modes_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, D, k, nlist = args.n, args.dim, args.topk, args.nlist
    base = synth.make_clustered_vectors(n, D, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, D, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=n, dim=D, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters)
    cents, _ = api.train_ivf_centroids(base, nlist, max_iters=args.train_iters)
    labels, _ = api.ivf_assign(cents, base)
    labels = labels.astype(np.int32)
    rng = np.random.default_rng(5)
    masks = {pct: rng.random(n) < share if share < 1 else np.ones(n, dtype=bool) for pct, share in SHARES}
    lo, hi = float(base.min()), float(base.max())
    as_bytes = lambda a: np.clip(np.rint((a - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    thr = base.mean(axis=0).astype(np.float32)
    with api.FlatIndex(base) as ref, api.FlatIVF.from_labels(ref, labels, nlist, centroids=cents) as coarse:
        probes = {p: torch.from_numpy(coarse.probe(qs, p)[0]).cuda() for p in args.nprobe}
    opened = {"f32": lambda: (api.FlatIndex(base), api.FlatIVF, qs),
              "u8": lambda: (api.FlatIndexU8(as_bytes(base)), api.FlatIVFBytes, as_bytes(qs)),
              "bits": lambda: (api.FlatIndexBits(api.bits_from_float(base, thr), D), api.FlatIVFBits, api.bits_from_float(qs, thr))}
    scale = 255.0 / (hi - lo)
    half = lambda a: api.FlatIndexHalf(a, "f16")
    ip_opened = {"f32": lambda: (api.FlatIndex(base), api.FlatIVF, qs, cents),
                 "f16": lambda: (half(base), api.FlatIVF, qs, cents),
                 "sq8": lambda: (api.FlatIndexSQ.from_float(base, bits=8), api.FlatIVF, qs, cents),
                 "u8": lambda: (api.FlatIndexU8(as_bytes(base)), api.FlatIVFBytes, as_bytes(qs), ((cents - lo) * scale).astype(np.float32)),
                 "i8": lambda: (api.FlatIndexI8((as_bytes(base).astype(np.int16) - 128).astype(np.int8)), api.FlatIVFBytes,
                                (as_bytes(qs).astype(np.int16) - 128).astype(np.int8), ((cents - lo) * scale - 128).astype(np.float32))}
    out["ip"] = {}
    for fmt in args.ip_formats:
        flat, cls, q, c = ip_opened[fmt]()
        d_q = torch.from_numpy(q).cuda()
        res = out["ip"][fmt] = {}
        with flat, cls.from_labels(flat, labels, nlist, centroids=c) as ivf:
            res["flat_search_ip_host_ms"] = taking_turns({"flat_search_ip": lambda: flat.search_ip(q, k)}, 3)["flat_search_ip"]
            for p in args.nprobe:
                d_l2 = torch.from_numpy(ivf.probe(q, p)[0]).cuda()  # the scan's cost per row: both metrics over the SAME lists
                res["nprobe_%d" % p] = taking_turns({"search_l2": lambda: ivf.search_torch(d_q, p, k),
                                                     "search_ip": lambda: ivf.search_ip_torch(d_q, p, k),
                                                     "probes_l2": lambda: ivf.search_probes_torch(d_q, d_l2, k),
                                                     "probes_ip": lambda: ivf.search_probes_ip_torch(d_q, d_l2, k)}, args.reps)
    for kind in args.kinds:
        flat, cls, q = opened[kind]()
        d_q = torch.from_numpy(q).cuda()
        res = out[kind] = {}
        with flat, cls.from_labels(flat, labels, nlist) as ivf:
            filters = {pct: api.FlatIdFilter.from_mask(flat, m) for pct, m in masks.items()}
            res["flat_filtered_host_ms"] = taking_turns(
                {"flat_filtered_" + pct: (lambda f=f: flat.search_filtered(q, k, f)) for pct, f in filters.items()}, 3)
            for p, d_probes in probes.items():
                fns = {"unfiltered": lambda: ivf.search_probes_torch(d_q, d_probes, k)}
                for pct, f in filters.items():
                    fns["filtered_" + pct] = lambda f=f: ivf.search_probes_torch(d_q, d_probes, k, id_filter=f)
                a, b = fns["unfiltered"](), fns["filtered_100"]()
                res["nprobe_%d" % p] = dict(same_as_cut_lists=bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])),
                                            call_ms=taking_turns(fns, args.reps))
            for f in filters.values():
                f.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
