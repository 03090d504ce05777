#!/usr/bin/env python
"""Measurements of the search by distance tables and of the inner-product search on the bench index
(bench.py's pipeline recipe: clustered vectors -> k-means codebook -> PQ codes -> DeltaTree); writes one JSON object
(default profiles/tables_ip_line.json) and prints it.

  steps     synchronous query_batch_torch(queries), query_batch_tables_torch(their L2 tables) and query_batch_ip_torch
            (queries), alternating --rounds times, --reps calls a round, host clock around a synchronised call; the median
            of the rounds' medians.  The L2 tables are made on the device by the table rule itself (fp32 subtract, fp64
            square, float += double), and the two L2 answers are compared to the bit before anything is timed.
  counters  exact checks and candidates per query from dpq_profile for the L2 call and the inner-product call: a
            bootstrap steered by L2 neighbour lists would show here.
  recall    recall@topk of the PQ inner-product answer against torch's matmul + topk over the raw vectors.  The torch
            side is fp32 GEMM arithmetic: a ground truth, not a bit-exact reference.
Kernel times of tables_ingest_kernel and lut_build_kernel come from a kernel-trace run of this script of its own
(--trace-only: the three calls a few times, nothing timed by the host).
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


def note(msg):
    print("[dev_tables_search] " + msg, file=sys.stderr, flush=True)


def l2_tables_torch(cb, q):
    """[nq][M][K] float32 on the device by the L2 table rule: acc32 = float32(float64(acc32) + float64(diff32)^2)."""
    import torch
    M, K, Ds = cb.shape
    qs = q.reshape(q.shape[0], M, Ds)
    acc = torch.zeros((q.shape[0], M, K), dtype=torch.float32, device=q.device)
    for d in range(Ds):
        diff = cb[None, :, :, d] - qs[:, :, None, d]
        acc = (acc.double() + diff.double() * diff.double()).float()
    return acc.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--flags", type=int, default=0, help="dpq_open_opts.flags (8 = DPQ_OPT_BOOT_FULLSORT: cells ordered by the tables alone)")
    ap.add_argument("--cache", default="", help="npz file that keeps the built index (codebook, payload, vec_id) between runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_ip_line.json"))
    args = ap.parse_args()
    import torch
    n, nq, k, M, D = args.n, args.queries, args.topk, 8, 128

    t0 = time.time()
    base = synth.make_clustered_vectors(n, D, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    if args.cache and os.path.exists(args.cache):
        z = np.load(args.cache)
        cb, payload, vec_id = z["codebook"], z["payload"], z["vec_id"]
    else:
        cb = synth.kmeans_codebook(base, M, 256, iters=6, seed=102)
        codes = api.encode_pq(base, cb, device=0)
        tree = api.DeltaTree(codes, codebook=cb, device=0)
        payload, vec_id = tree.payload(), tree.vec_id.astype(np.int64)
        tree.close()
        if args.cache:
            np.savez(args.cache, codebook=cb, payload=payload, vec_id=vec_id)
    qs = synth.make_clustered_vectors(nq, D, seed=1, n_clusters=20000, spread=12.0, centre_seed=7)
    note("index of %d codes built in %.1f s" % (n, time.time() - t0))

    dev = torch.device("cuda", 0)
    d_q = torch.from_numpy(qs).to(dev)
    d_cb = torch.from_numpy(cb).to(dev)
    out = dict(n=n, queries=nq, topk=k, M=M, rounds=args.rounds, reps=args.reps, flags=args.flags)
    with api.DeltaPQIndex.open_memory(payload, n, M, 256, device=0, flags=args.flags) as idx:
        idx.set_codebook(cb)
        d_tab = l2_tables_torch(d_cb, d_q)
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dd = torch.empty((nq, k), dtype=torch.float32, device=dev)
        calls = dict(l2_queries=lambda: idx.query_batch_torch(d_q, k, out_ids=ids, out_dists=dd),
                     l2_tables=lambda: idx.query_batch_tables_torch(d_tab, k, out_ids=ids, out_dists=dd),
                     ip=lambda: idx.query_batch_ip_torch(d_q, k, out_ids=ids, out_scores=dd))
        a = [t.clone() for t in calls["l2_queries"]()]
        b = [t.clone() for t in calls["l2_tables"]()]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), \
            "query_batch_tables_torch on the L2 tables differs from query_batch_torch on the queries"
        out["l2_tables_equal_l2_queries"] = True
        if args.trace_only:
            for _ in range(5):
                for fn in calls.values():
                    fn()
            torch.cuda.synchronize()
            return
        for fn in calls.values():                       # warm-up: plans, workspaces, the plain-code image
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        series = {name: [] for name in calls}
        for _ in range(args.rounds):                    # alternating, so that clock and thermal drift hit all three alike
            for name, fn in calls.items():
                ts = []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    fn()                                # synchronous: returns with the results complete
                    ts.append((time.perf_counter() - t) * 1e3)
                series[name].append(statistics.median(ts))
        out["step_ms_rounds"] = {name: [round(v, 4) for v in s] for name, s in series.items()}
        out["step_ms"] = {name: round(statistics.median(s), 4) for name, s in series.items()}
        out["queries_per_s"] = {name: round(nq / (statistics.median(s) * 1e-3)) for name, s in series.items()}

        idx.profile_enable(True)
        out["per_query"] = {}
        for name in ("l2_queries", "ip"):
            idx.profile_reset()
            calls[name]()
            p = idx.profile_read()
            out["per_query"][name] = dict(exact_checks=round(p["exact_checks"] / nq, 1), candidates=round(p["candidates"] / nq, 1),
                                          overflow_reruns=p["overflow_reruns"])
        idx.profile_enable(False)

        pos, scores = idx.query_batch_ip_torch(d_q, k)
        pos = pos.cpu().numpy().astype(np.int64)
    pos = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    found = np.where(pos >= 0, vec_id[np.maximum(pos, 0)], -1)
    d_base = torch.from_numpy(base).to(dev)
    truth = torch.topk(d_q @ d_base.T, k, dim=1).indices.cpu().numpy()     # fp32 GEMM: not bit-exact, a ground truth
    hits = sum(len(np.intersect1d(found[i], truth[i])) for i in range(nq))
    out["ip_recall_at_topk_vs_torch_matmul"] = round(hits / (nq * k), 4)
    out["note"] = "recall: PQ inner-product top-%d against torch matmul top-%d over the raw vectors (fp32 GEMM, not bit-exact)" % (k, k)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
