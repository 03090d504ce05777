#!/usr/bin/env python
"""Measurements of the exact search over 8-bit and 4-bit scalar-quantised vectors beside the fp32 and
the f16 handle, in one run, on the bench-shaped vectors of scripts/dev_exact_half.py; prints one JSON line and writes it to
`--out`.

  quantiser  dpq_sq_train and dpq_sq_encode for both widths
  open       dpq_flat_open (fp32), dpq_flat_open_sq (codes the caller has) and dpq_flat_open_quantised (fp32 rows, trained
             and encoded on the GPU) for both widths; the device bytes of each handle's rows
  search     exact top-`--topk` of `--nq` queries over all `--n` vectors by L2 and by inner product on the fp32, the sq8 and
             the sq4 handle; whether each quantised answer equals the fp32 handle's over the decoded rows, bit for bit; and
             recall@topk of the search over the quantised rows against the fp32 truth
  rerank     the index of DESIGN.md 5.14 (synth.kmeans_codebook, six rounds), its PQ top-`--rerank` by L2 and by inner
             product, the exact re-rank of those answers to top-`--topk` on device tensors on the fp32, f16, sq8 and sq4
             handles, and recall@topk of every re-ranked answer against the fp32 handle's exact search
Every timing is `--reps` calls after a warm-up call, median and min - max on the host clock around the call.
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

WIDTHS = (("sq8", 8), ("sq4", 4))


def spread(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def timed(fn, reps):
    fn()  # warm-up: workspaces, code objects
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rerank", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_sq_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    import torch
    base = synth.make_clustered_vectors(args.n, args.dim, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    qs = synth.make_clustered_vectors(args.nq, args.dim, seed=1, n_clusters=20000, spread=12.0, centre_seed=7)
    out = dict(n=args.n, dim=args.dim, nq=args.nq, top_k=args.topk, rerank=args.rerank, reps=args.reps)

    def opened(make):
        make().close()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            h = make()
            ms.append((time.perf_counter() - t0) * 1e3)
            h.close()
        return spread(ms)

    quant, stored = {}, {}
    for name, bits in WIDTHS:
        quant[name], ms = timed(lambda: api.sq_train(base, bits), args.reps)
        out["train_%s_ms" % name] = spread(ms)
        stored[name], ms = timed(lambda: api.sq_encode(base, *quant[name], bits), args.reps)
        out["encode_%s_ms" % name] = spread(ms)
        out["step_range_%s" % name] = [float(quant[name][1].min()), float(quant[name][1].max())]
    out["open_fp32_ms"] = opened(lambda: api.FlatIndex(base))
    for name, bits in WIDTHS:
        out["open_sq_%s_ms" % name] = opened(lambda: api.FlatIndexSQ(stored[name], *quant[name], bits))
        out["open_quantised_%s_ms" % name] = opened(lambda: api.FlatIndexSQ.from_float(base, bits))
    pad = lambda d, m: (d + m - 1) // m * m
    out["device_bytes"] = dict(fp32=4 * args.n * pad(args.dim, 4), f16=2 * args.n * pad(args.dim, 8),
                               sq8=args.n * pad(args.dim, 16) + 8 * pad(args.dim, 32),
                               sq4=args.n * pad(args.dim, 32) // 2 + 8 * pad(args.dim, 32))

    handles = {"fp32": api.FlatIndex(base), "f16": api.FlatIndexHalf(base, "f16")}
    for name, bits in WIDTHS:
        handles[name] = api.FlatIndexSQ.from_float(base, bits)
    truth = {}
    for name, h in handles.items():
        if name == "f16":  # its search is DESIGN.md 5.10.4's; here it is the re-rank's yardstick
            continue
        res_l2, ms = timed(lambda: h.search(qs, args.topk), args.reps)
        out["search_l2_%s_call_ms" % name] = spread(ms)
        res_ip, ms = timed(lambda: h.search_ip(qs, args.topk), args.reps)
        out["search_ip_%s_call_ms" % name] = spread(ms)
        if name == "fp32":
            truth = {"l2": res_l2, "ip": res_ip}
        else:
            bits = dict(WIDTHS)[name]
            lo, step, _ = h.quantiser()
            with api.FlatIndex(api.sq_decode(stored[name], lo, step, bits)) as wide:
                out["search_%s_equals_fp32_over_decoded" % name] = same(res_l2, wide.search(qs, args.topk)) and \
                    same(res_ip, wide.search_ip(qs, args.topk))
            out["search_l2_%s_recall_at_%d" % (name, args.topk)] = api.recall(res_l2[0], truth["l2"][0], k=args.topk, R=args.topk)
            out["search_ip_%s_recall_at_%d" % (name, args.topk)] = api.recall(res_ip[0], truth["ip"][0], k=args.topk, R=args.topk)

    cb = synth.kmeans_codebook(base, 8, 256, iters=6, seed=102)
    codes = api.encode_pq(base, cb, device=0)
    tree = api.DeltaTree(codes, codebook=cb, device=0)
    with api.DeltaPQIndex.open_memory(tree.payload(), args.n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        pos = {"l2": idx.query_batch(qs, args.rerank)[0], "ip": idx.query_batch_ip(qs, args.rerank)[0]}
    d_q = torch.from_numpy(qs).cuda()
    for name, h in handles.items():
        h.set_id_map(tree.vec_id)
        for metric, call in (("l2", h.rerank_torch), ("ip", h.rerank_ip_torch)):
            d_c = torch.from_numpy(pos[metric]).cuda()

            def on_device():
                r = call(d_q, d_c, args.topk)
                torch.cuda.synchronize()
                return r
            (ti, _), ms = timed(on_device, args.reps)
            out["rerank_%s_%s_device_call_ms" % (metric, name)] = spread(ms)
            out["reranked_%s_%s_recall_at_%d" % (metric, name, args.topk)] = api.recall(ti.cpu().numpy(), truth[metric][0],
                                                                                        k=args.topk, R=args.topk)
        h.close()
    tree.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
