"""What building a search filter costs, host path against device constructors, on the bench's index (GPU box): the
pipeline-built 1 M codes, M = 8 (so that a real DFS position -> vector id map exists), at 100 %, 10 % and 0.1 % of the
ids allowed.

Prints one JSON line.  Per density, the median of --reps alternating runs (ms, wall time of the call unless said
otherwise):
  host.*     the path as it was before the device constructors: bitmap_to_dfs + dpq_filter_create from a bitmap over
             vector ids, pack_ids + dpq_filter_create from an id list, dpq_filter_create alone from a ready bitmap
  device.*   each device constructor from inputs that already live on the GPU: wall time of the call, and `_kernel_ms`
             between two hipEvents around it (the call's kernels and its count read-back, without the host's share)
  query_ms   query_batch_filtered (1000 queries, top-100) through the same filter, for scale
--stream-n N > 0 adds the same at N codes of a synthetic stream (bench.py --data stream's shape; no builder ran, so the
map is a random permutation).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deltapq_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--stream-n", type=int, default=0)
ap.add_argument("--stream-reps", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()


def timed(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def close_after(build):
    def run():
        build().close()
    return run


def measure(idx, n, vec, queries, reps):
    N = idx.info()["n_codes_total"]
    n_ids = n + 1                                        # reported ids 0 .. N (the even-N rule)
    res = {}
    for frac in (1.0, 0.1, 0.001):
        rng = np.random.default_rng(7)
        mask = np.ones(n_ids, dtype=bool) if frac == 1.0 else rng.random(n_ids) < frac
        if N % 2 == 0:
            mask[N - 1] = False                          # (names nothing)
        rep = np.arange(n, dtype=np.int64)
        if N % 2 == 0:
            rep[N - 1] = N
        vmask = np.zeros(n, dtype=bool)
        vmask[vec] = mask[rep]
        ids = np.flatnonzero(mask).astype(np.int32)
        words, nb = api.IdFilter.pack_mask(mask)
        vwords, vnb = api.IdFilter.pack_mask(vmask)
        d_mask, d_vmask, d_ids = torch.from_numpy(mask).cuda(), torch.from_numpy(vmask).cuda(), torch.from_numpy(ids).cuda()
        d_vids = torch.from_numpy(np.flatnonzero(vmask).astype(np.int32)).cuda()
        lo, hi = 0, max(1, int(frac * n_ids))

        def host_vec():
            w, b = api.bitmap_to_dfs(vwords, vnb, vec)
            api.IdFilter(idx, w, b).close()

        runs = {
            "host.vec_bitmap": host_vec,
            "host.id_list": lambda: api.IdFilter(idx, *api.IdFilter.pack_ids(ids, n_ids)).close(),
            "host.ready_bitmap": lambda: api.IdFilter(idx, words, nb).close(),
            "device.mask": close_after(lambda: api.IdFilter.from_mask_torch(idx, d_mask)),
            "device.ids": close_after(lambda: api.IdFilter.from_ids_torch(idx, d_ids)),
            "device.ids_inverted": close_after(lambda: api.IdFilter.from_ids_torch(idx, d_ids, invert=True)),
            "device.range": close_after(lambda: api.IdFilter.from_range(idx, lo, hi)),
            "device.vec_mask": close_after(lambda: api.IdFilter.from_vec_mask_torch(idx, d_vmask)),
            "device.vec_ids": close_after(lambda: api.IdFilter.from_vec_ids_torch(idx, d_vids, n)),
            "host_input.ids": close_after(lambda: api.IdFilter.from_ids(idx, ids)),
            "host_input.vec_mask": close_after(lambda: api.IdFilter.from_vec_mask(idx, vmask)),
        }
        with api.IdFilter.from_mask(idx, mask) as fh, api.IdFilter.from_vec_mask_torch(idx, d_vmask) as fv, \
                api.IdFilter.from_ids_torch(idx, d_ids) as fi:
            assert fh.n_allowed == fv.n_allowed == fi.n_allowed, (fh.n_allowed, fv.n_allowed, fi.n_allowed)
            assert np.array_equal(fh.to_mask(n_ids), fv.to_mask(n_ids)) and np.array_equal(fh.to_mask(n_ids), fi.to_mask(n_ids))
            allowed = fh.n_allowed
            with fi & fv as both:
                runs["device.combine_and"] = close_after(lambda: fi & fv)
                assert both.n_allowed == allowed
            for fn in runs.values():                     # warm-up
                fn()
            idx.query_batch_filtered(queries, args.k, fv)
            wall = {name: [] for name in runs}
            kern = {name: [] for name in runs if name.startswith("device.")}
            t_q = []
            for _ in range(reps):                        # alternating: every path sees the same drift
                for name, fn in runs.items():
                    wall[name].append(timed(fn))
                for name in kern:
                    kern[name].append(event_timed(runs[name]))
                t_q.append(timed(lambda: idx.query_batch_filtered(queries, args.k, fv)))
        row = {"allowed": allowed}
        for name in runs:
            row[name + "_ms"] = round(float(np.median(wall[name])), 4)
        for name in kern:
            row[name + "_kernel_ms"] = round(float(np.median(kern[name])), 4)
        row["query_ms"] = round(float(np.median(t_q)), 4)
        res["%g%%" % (100 * frac)] = row
        print("n=%d %g%%: %s" % (n, 100 * frac, json.dumps(row)), file=sys.stderr, flush=True)
    return res


out = {"queries": args.queries, "k": args.k, "reps": args.reps}
t0 = time.time()
base = synth.make_clustered_vectors(args.n, 128, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
cb = synth.kmeans_codebook(base, 8, 256, iters=6, seed=102)
codes = api.encode_pq(base, cb)
del base
tree = api.DeltaTree(codes, codebook=cb, device=0)
payload, vec = tree.payload(), tree.vec_id.copy()
tree.close()
queries = synth.make_clustered_vectors(args.queries, 128, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
out["setup_s"] = round(time.time() - t0, 1)
print("bench index built in %.1f s" % out["setup_s"], file=sys.stderr, flush=True)
with api.DeltaPQIndex.open_memory(payload, args.n, 8, 256) as idx:
    idx.set_codebook(cb)
    idx.set_vec_ids(vec)
    out["bench_index"] = {"n": args.n, "density": measure(idx, args.n, vec, queries, args.reps)}
if args.stream_n > 0:
    t0 = time.time()
    cb2 = synth.make_codebook(8, 256, 16, seed=100)
    payload2, _ = synth.encode_dtc(synth.synth_tree_large(args.stream_n, 8, seed=102, mean_diffs=3.0))
    vec2 = np.random.default_rng(3).permutation(args.stream_n).astype(np.uint32)
    q2 = synth.make_queries(args.queries, 128, seed=101)
    print("stream of %d codes made in %.1f s" % (args.stream_n, time.time() - t0), file=sys.stderr, flush=True)
    with api.DeltaPQIndex.open_memory(payload2, args.stream_n, 8, 256) as idx:
        idx.set_codebook(cb2)
        idx.set_vec_ids(vec2)
        out["stream_index"] = {"n": args.stream_n, "setup_s": round(time.time() - t0, 1),
                               "density": measure(idx, args.stream_n, vec2, q2, args.stream_reps)}
line = json.dumps(out)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
