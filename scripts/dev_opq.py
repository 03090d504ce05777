#!/usr/bin/env python
"""Measurements of OPQ; writes one JSON object (default profiles/opq_line.json) and prints it.

Parts (--parts, comma separated):
  bench       the bench vectors (a clipped Gaussian mixture): PQ against OPQ from the same seed and the same number of
              Lloyd rounds -- objective per outer step, recall@topk against the exact search over the raw vectors, DTC
              payload bytes of both indexes, wall time and per-phase milliseconds of dpq_opq_train
  correlated  the same lines on the correlated data of tests/test_opq.py at --n x --dim
  rotate      dpq_rotate_device at 1000 x dim and n x dim, device events, median of five
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


def correlated(n, dim, z_seed):
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    z = np.random.default_rng(z_seed).standard_normal((n, dim)) * 0.8 ** np.arange(dim)
    return (z @ Q).astype(np.float32)


def index_recall(base, qs, truth, cb, k, rotation=None):
    """(recall@k, DTC payload bytes) of the index over `base` (rotated first when a rotation is given)."""
    n = base.shape[0]
    codes = api.encode_pq(base if rotation is None else api.rotate(base, rotation), cb)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    with api.DeltaPQIndex.open_memory(payload, n, cb.shape[0], cb.shape[1], device=0) as idx:
        idx.set_codebook(cb)
        searcher = idx if rotation is None else api.RotatedIndex(idx, rotation)
        pos, _ = searcher.query_batch(qs, k)
    pos = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    found = np.where(pos >= 0, tree.vec_id[np.maximum(pos, 0)].astype(np.int64), -1).astype(np.int32)
    rec = api.recall(found, truth, k=k, R=k)
    tree.close()
    return rec, int(len(payload))


def note(msg):
    print("[dev_opq] " + msg, file=sys.stderr, flush=True)


def compare(base, qs, args):
    k = args.topk
    sample = base[:args.train]
    t0 = time.perf_counter()
    R, cb, st = api.train_opq(sample, 8, 256, outer_iters=args.outer, init_iters=args.init_iters, inner_iters=args.inner_iters,
                              seed=0)
    wall = time.perf_counter() - t0
    note("trained OPQ in %.1f s, objective %s" % (wall, st["objective"]))
    rounds = args.init_iters + args.outer * args.inner_iters
    plain, _ = api.train_codebook(sample, 8, 256, max_iters=min(64, rounds), seed=0)
    with api.FlatIndex(base) as flat:
        truth, _ = flat.search(qs, k)
    note("exact search done")
    pq_rec, pq_bytes = index_recall(base, qs, truth, plain, k)
    note("PQ recall %.4f" % pq_rec)
    opq_rec, opq_bytes = index_recall(base, qs, truth, cb, k, rotation=R)
    return dict(n=int(base.shape[0]), dim=int(base.shape[1]), train=int(sample.shape[0]), outer_iters=args.outer,
                init_iters=args.init_iters, inner_iters=args.inner_iters, plain_rounds=min(64, rounds),
                objective=st["objective"], best_t=st["best_t"], degenerate=st["degenerate"],
                rotation_residual_max=max(st["rotation_residual"] or [0.0]),
                plain_objective=float(sum(api.train_potential(sample, plain))),
                **{"pq_recall_at_%d" % k: pq_rec, "opq_recall_at_%d" % k: opq_rec},
                pq_dtc_bytes=pq_bytes, opq_dtc_bytes=opq_bytes, opq_train_wall_s=wall,
                opq_train_ms={f: st[f] for f in ("wall_ms", "gpu_ms", "rounds_ms", "assign_ms", "update_ms", "repair_ms",
                                                 "rotate_ms", "cross_ms", "procrustes_ms")})


def rotate_times(n, dim):
    import torch
    out = {}
    R = torch.from_numpy(np.linalg.qr(np.random.default_rng(1).standard_normal((dim, dim)))[0].astype(np.float32)).cuda()
    for rows in (1000, n):
        x = torch.randn((rows, dim), dtype=torch.float32, device="cuda")
        y = torch.empty_like(x)
        api.rotate_torch(x, R, out=y)   # warm-up: code object
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            api.rotate_torch(x, R, out=y)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out["%dx%d" % (rows, dim)] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                                          bytes_moved=2 * rows * dim * 4, fp64_fma=rows * dim * dim)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--train", type=int, default=65536)
    ap.add_argument("--outer", type=int, default=8)
    ap.add_argument("--init-iters", type=int, default=25)
    ap.add_argument("--inner-iters", type=int, default=4)
    ap.add_argument("--parts", default="rotate,bench,correlated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opq_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    out = {}
    if os.path.exists(args.out):        # parts run one at a time add to the same file
        out = json.load(open(args.out))
    for part in args.parts.split(","):
        if part == "rotate":
            out["rotate_device"] = rotate_times(args.n, args.dim)
        elif part == "bench":
            base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
            qs = synth.make_clustered_vectors(args.nq, args.dim, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
            out["bench_mixture"] = compare(base, qs, args)
        elif part == "correlated":
            out["correlated"] = compare(correlated(args.n, args.dim, 6), correlated(args.nq, args.dim, 7), args)
        else:
            raise SystemExit("unknown part " + part)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
