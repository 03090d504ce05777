#!/usr/bin/env python
"""Measurements of the IVF search by residual on the bench-shaped vectors; prints one JSON line, writes it
to --out, and asserts nothing.

Two indexes of the same M = 8, K = 256 over the same vectors, lists and centroids (train_ivf_centroids, ivf_assign): one
encodes the vectors, one their residuals x - c_list (ivf_residuals).  Per nprobe:
  recall   recall@top_k of IVF.search on the first and of IVF.search_residual on the second against the exact truth
           (FlatIndex.search over the raw vectors);
  call_ms  ms per synchronous call of search_residual_torch with the group P = 1, 2, 4 (DPQ_IVF_RESIDUAL_GROUP, read per
           call under DPQ_DEV=1) beside search_torch on the non-residual index, the calls taking turns: median [min - max]
           of --reps rounds.
--kernel-trace DIR: instead of timing, one call of each kind at --trace-nprobe, for a run under
`rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dev_ivf_residual.py --kernel-trace DIR ...`; the per-kernel
table is what rocprofv3 leaves in DIR.
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


def vector_ids(ids, vec_id, n):
    """Reported ids -> the vectors of their nodes (-1 stays): id n is node n - 1 of an even-N index."""
    pos = np.where(ids == n, n - 1, ids)
    return np.where(ids >= 0, vec_id[np.maximum(pos, 0)], -1).astype(np.int32)


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
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--trace-nprobe", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_residual_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    n, k, nlist = args.n, args.topk, args.nlist
    base = synth.make_clustered_vectors(n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=n, dim=args.dim, nq=args.nq, top_k=k, nlist=nlist, reps=args.reps, train_iters=args.train_iters, M=8, K=256)
    with api.FlatIndex(base) as flat:
        truth = flat.search(qs, k)[0]
    cents, _ = api.train_ivf_centroids(base, nlist, max_iters=args.train_iters)
    vec_labels, _ = api.ivf_assign(cents, base)
    d_q = torch.from_numpy(qs).cuda()
    opened = {}
    for name, rows in (("plain", base), ("residual", api.ivf_residuals(cents, base, vec_labels))):
        cb, _ = api.train_codebook(rows, 8, 256, max_iters=25, seed=0)
        tree = api.DeltaTree(api.encode_pq(rows, cb), codebook=cb, device=0)
        vec_id = tree.vec_id.astype(np.int64)
        idx = api.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0)
        idx.set_codebook(cb)
        opened[name] = (idx, api.IVF.from_labels(idx, vec_labels[vec_id], nlist, centroids=cents), vec_id)
        tree.close()
    (_, ivf_p, vid_p), (_, ivf_r, vid_r) = opened["plain"], opened["residual"]

    def residual_at(P, nprobe):
        def call():
            os.environ["DPQ_IVF_RESIDUAL_GROUP"] = str(P)
            return ivf_r.search_residual_torch(d_q, nprobe, k)
        return call

    if args.kernel_trace:
        calls = {"ivf_search": lambda: ivf_p.search_torch(d_q, args.trace_nprobe, k)}
        calls.update({"search_residual_P%d" % P: residual_at(P, args.trace_nprobe) for P in (1, 2, 4)})
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        out["kernel_trace"] = dict(nprobe=args.trace_nprobe, calls=list(calls), dir=os.path.basename(args.kernel_trace))
    else:
        for nprobe in args.nprobe:
            fns = {"ivf_search": lambda: ivf_p.search_torch(d_q, nprobe, k)}
            fns.update({"search_residual_P%d" % P: residual_at(P, nprobe) for P in (1, 2, 4)})
            answers = {name: fn()[0].cpu().numpy() for name, fn in fns.items()}
            out["nprobe_%d" % nprobe] = dict(
                recall_ivf_search=api.recall(vector_ids(answers["ivf_search"], vid_p, n), truth),
                recall_search_residual=api.recall(vector_ids(answers["search_residual_P4"], vid_r, n), truth),
                same_answer_for_every_P=bool(np.array_equal(answers["search_residual_P1"], answers["search_residual_P2"]) and
                                             np.array_equal(answers["search_residual_P1"], answers["search_residual_P4"])),
                call_ms=taking_turns(fns, args.reps))
    for idx, ivf, _ in opened.values():
        ivf.close()
        idx.close()
    line = json.dumps(out)
    print(line)
    if not args.kernel_trace:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
