"""Code lookup on the bench's index (GPU box): the pipeline-built 1 M codes, M = 8, Ds = 16; with --big N also a
synthetic N-code index (synth_tree_large, the bench's `--data stream` synthesis).

Prints one JSON line:
  bulk     dpq_decode_range over the whole handle, end to end (median of --reps calls): ms and GB/s of decoded codes
           arriving in host memory -- that figure is the PCIe copy, not the decode -- and, so that one
           `rocprofv3 --kernel-trace --stats -- python scripts/dev_lookup.py` run holds both launches of
           decode_list_kernel, a 256-query search batch (which decodes the same segments with the relabelling).
  random   for n in --sizes uniformly random reported ids, device tensors in and out, the synchronous call (kernels +
           the flag word's round trip) for codes and for reconstructed vectors, each three ways: the per-request
           kernel alone (DPQ_LOOKUP_GROUPED=0), the grouped path alone (=1: every segment decoded once, then a row
           gather), and the library's own choice; ids/s and the reconstruction's output bandwidth (n * M * Ds * 4
           bytes / time) of the library's choice; and the baseline "decode the whole handle, then gather rows" done
           by the caller: decode_range (kernel + copy to the host), the copy back, a torch row gather.
Kernel times come from the rocprofv3 run's trace (lookup_kernel, gather_codes_kernel, decode_list_kernel rows).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["DPQ_DEV"] = "1"                                # DPQ_LOOKUP_GROUPED is a developer switch
import numpy as np
import torch

from deltapq_amd import api, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--big", type=int, default=0, help="also measure a synthetic index of this many codes (e.g. 125000000)")
ap.add_argument("--sizes", default="1,1000,100000,1000000,10000000")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def median_ms(fn, reps):
    fn()                                                   # warm-up: allocations, code object load
    fn()
    return 1e3 * float(np.median([timed(fn) for _ in range(reps)]))


def measure(idx, cb, n_codes, queries, label):
    inf = idx.info()
    M, Ds = inf["M"], inf["Ds"]
    out = {"n_codes": n_codes, "bulk": {}, "random": {}}
    ms = median_ms(lambda: idx.decode_range(), max(3, args.reps // 4))
    out["bulk"] = {"decode_range_ms": round(ms, 3), "host_GBps": round(n_codes * M / ms / 1e6, 3)}
    if queries is not None:
        idx.query_batch(queries[:256], 100)
        out["bulk"]["search_256q_ms"] = round(median_ms(lambda: idx.query_batch(queries[:256], 100), 5), 3)
    full = torch.from_numpy(idx.decode_range()).cuda()
    host_full = full.cpu().numpy()
    up_ms = median_ms(lambda: torch.from_numpy(host_full).cuda(), 5)         # the baseline's copy back to the device
    rng = np.random.default_rng(1)

    def paths(fn, reps):
        res = {}
        for name, env in (("per_request", "0"), ("grouped", "1"), ("auto", None)):
            if env is None:
                os.environ.pop("DPQ_LOOKUP_GROUPED", None)
            else:
                os.environ["DPQ_LOOKUP_GROUPED"] = env
            res[name] = median_ms(fn, reps)
        os.environ.pop("DPQ_LOOKUP_GROUPED", None)
        return res

    for n in sizes:
        ids = rng.integers(0, n_codes - 1, size=n).astype(np.int32)          # (never the N - 1 hole)
        t = torch.from_numpy(ids).cuda()
        codes = torch.empty((n, M), dtype=torch.uint8, device="cuda")
        vecs = torch.empty((n, M * Ds), dtype=torch.float32, device="cuda")
        reps = args.reps if n <= 1_000_000 else max(3, args.reps // 4)
        c = paths(lambda: idx.get_codes_torch(t, out=codes), reps)
        v = paths(lambda: idx.reconstruct_torch(t, out=vecs), reps)
        tl = t.long()
        g_ms = median_ms(lambda: full.index_select(0, tl), reps)
        assert torch.equal(full.index_select(0, tl), codes)
        out["random"][str(n)] = {
            "codes_ms": {k: round(x, 4) for k, x in c.items()}, "codes_ids_per_s": round(n / c["auto"] * 1e3),
            "reconstruct_ms": {k: round(x, 4) for k, x in v.items()},
            "reconstruct_ids_per_s": round(n / v["auto"] * 1e3),
            "reconstruct_out_GBps": round(n * M * Ds * 4 / v["auto"] / 1e6, 2),
            "baseline_decode_all_ms": round(ms + up_ms, 3), "baseline_gather_ms": round(g_ms, 4)}
        del codes, vecs, t, tl
    print(label, json.dumps(out), flush=True)
    return out


t0 = time.time()
base = synth.make_clustered_vectors(args.n, 128, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
cb = synth.kmeans_codebook(base, 8, 256, iters=6, seed=102)
codes = api.encode_pq(base, cb)
del base
tree = api.DeltaTree(codes, codebook=cb, device=0)
payload = tree.payload()
tree.close()
queries = synth.make_clustered_vectors(256, 128, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
result = {"setup_s": round(time.time() - t0, 1), "reps": args.reps}
with api.DeltaPQIndex.open_memory(payload, args.n, 8, 256) as idx:
    idx.set_codebook(cb)
    result["bench_index"] = measure(idx, cb, args.n, queries, "bench_index")
if args.big:
    t0 = time.time()
    big = synth.synth_tree_large(args.big, 8, seed=5)
    payload, _ = synth.encode_dtc(big)
    del big
    with api.DeltaPQIndex.open_memory(payload, args.big, 8, 256) as idx:
        idx.set_codebook(cb)
        result["big_setup_s"] = round(time.time() - t0, 1)
        result["big_index"] = measure(idx, cb, args.big, None, "big_index")
print(json.dumps(result), flush=True)
