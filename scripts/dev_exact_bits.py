#!/usr/bin/env python
"""Measurements of the exact Hamming search over packed binary vectors beside the byte handle over rows
of the same byte length, in one run; prints one JSON line and writes it to `--out`.

  data       `--n` rows of `--bits` bits: fp32 normals binarised at zero (dpq_bits_from_float), `--nq` queries made the same way
  open       dpq_flat_open_bits (the packed rows), dpq_flat_open_binarised (the fp32 rows), dpq_flat_open_u8 (the packed
             rows read as `--bits` / 8 byte dimensions); the device bytes of each handle's rows
  search     exact top-`--topk` over all rows; the same under a filter that allows 10 % and 0.1 % of the rows; range search
             at the median distance of the `--topk`-th neighbour; device re-rank of `--rerank` random candidates per query
Every search figure is the median (and min - max) of `--reps` calls on the host clock, the bits handle and the byte handle
called in turn; the calls end with their answers on the host (re-rank: a device synchronise).
`--profile`: no timing; the bits handle only, `--profile-calls` top-k calls and one range call -- the process to put under
rocprofv3 for kernel times or counters.
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
from deltapq_amd import api  # noqa: E402


def spread(vals):
    return dict(median=statistics.median(vals), min=min(vals), max=max(vals))


def same(a, b):
    return bool(all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                    for x, y in zip(a, b)))


def alternating(calls, reps):
    """calls: name -> function.  A warm-up call each, then `reps` rounds in which every function is called once."""
    last = {name: fn() for name, fn in calls.items()}
    ms = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            last[name] = fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return last, {name: spread(v) for name, v in ms.items()}


def normals(rows, dim, seed):
    """fp32 [rows][dim], made in slices so that no fp64 copy of the whole array exists."""
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=np.float32)
    for r0 in range(0, rows, 65536):
        out[r0:r0 + 65536] = rng.standard_normal((min(65536, rows - r0), dim), dtype=np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--bits", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--rerank", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--open-reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_bits_line.json"))
    args = ap.parse_args()
    if args.bits % 8:
        raise SystemExit("--bits must be a multiple of 8: the byte handle beside it has --bits / 8 dimensions")
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    n, D, nq, nb = args.n, args.bits, args.nq, args.bits // 8
    rng = np.random.default_rng(3)

    if args.profile:
        base = rng.integers(0, 256, size=(n, nb), dtype=np.uint8)
        qs = rng.integers(0, 256, size=(nq, nb), dtype=np.uint8)
        with api.FlatIndexBits(base, D) as f:
            for _ in range(args.profile_calls):
                _, d = f.search(qs, args.topk)
            lims = f.range_search(qs, float(np.median(d[:, -1])))[0]
        print(json.dumps(dict(profile=True, n=n, bits=D, nq=nq, top_k=args.topk, range_keys=int(lims[-1]))))
        return

    import torch
    out = dict(n=n, bits=D, row_bytes=nb, nq=nq, top_k=args.topk, rerank=args.rerank, reps=args.reps, open_reps=args.open_reps)
    base_f = normals(n, D, 100)
    qs = api.bits_from_float(normals(nq, D, 1))
    t0 = time.perf_counter()
    base = api.bits_from_float(base_f)
    out["bits_from_float_ms"] = (time.perf_counter() - t0) * 1e3

    def opened(make):
        make().close()
        ms = []
        for _ in range(args.open_reps):
            t0 = time.perf_counter()
            h = make()
            ms.append((time.perf_counter() - t0) * 1e3)
            h.close()
        return spread(ms)

    out["open_bits_ms"] = opened(lambda: api.FlatIndexBits(base, D))
    out["open_binarised_ms"] = opened(lambda: api.FlatIndexBits.from_float(base_f))
    out["open_u8_ms"] = opened(lambda: api.FlatIndexU8(base))
    pad = lambda d, m: (d + m - 1) // m * m
    out["device_bytes"] = dict(bits=n * pad(nb, 16), u8=n * pad(nb, 32) + 4 * pad(n, 4), u8_of_unpacked_bits=n * pad(D, 32) + 4 * pad(n, 4))

    with api.FlatIndexBits.from_float(base_f) as fb:
        del base_f
        f, u = api.FlatIndexBits(base, D), api.FlatIndexU8(base)
        res, out["search_call_ms"] = alternating({"bits": lambda: f.search(qs, args.topk), "u8": lambda: u.search(qs, args.topk)}, args.reps)
        out["binarised_handle_equals_bits_handle"] = same(fb.search(qs, args.topk), res["bits"])
    radius = {name: float(np.median(r[1][:, -1])) for name, r in res.items()}
    out["range_radius"] = radius
    for frac in (0.1, 0.001):
        mask = rng.random(n) < frac
        ff, uf = api.FlatIdFilter.from_mask(f, mask), api.FlatIdFilter.from_mask(u, mask)
        _, out["search_filtered_%g_call_ms" % frac] = alternating(
            {"bits": lambda: f.search_filtered(qs, args.topk, ff), "u8": lambda: u.search_filtered(qs, args.topk, uf)}, args.reps)
        out["filter_%g_rows" % frac] = ff.n_allowed
        ff.close()
        uf.close()
    res, out["range_call_ms"] = alternating({"bits": lambda: f.range_search(qs, radius["bits"]),
                                             "u8": lambda: u.range_search(qs, radius["u8"])}, args.reps)
    out["range_keys"] = {name: int(r[0][-1]) for name, r in res.items()}
    d_q = torch.from_numpy(qs).cuda()
    d_c = torch.from_numpy(rng.integers(0, n, size=(nq, args.rerank)).astype(np.int32)).cuda()

    def on_device(h):
        r = h.rerank_torch(d_q, d_c, args.topk)
        torch.cuda.synchronize()
        return r
    _, out["rerank_device_call_ms"] = alternating({"bits": lambda: on_device(f), "u8": lambda: on_device(u)}, args.reps)
    f.close()
    u.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
