#!/usr/bin/env python
"""Measurements of the exact inner product over byte vectors in one run, on `--n` x `--dim` random
bytes with `--nq` queries and top-`--topk`; prints one JSON line and writes it to `--out`.

  search   search_ip on the u8 handle (dpq_flat_search_ip_u8), on the i8 handle over the same bytes minus 128
           (dpq_flat_search_ip_i8) and on the fp32 handle over the widened rows (dpq_flat_search_ip), with the L2 search of
           the u8 handle (dpq_flat_search_u8) beside them; whether the u8 answer equals the fp32 handle's, bit for bit
  bytes    the device bytes of each handle's rows and per-row arrays
  first    what the first inner-product call of a u8 handle costs beyond a later one: the row sums (one pass over the
           stored rows, 4 n bytes) and the queries' sums buffer.  The handle has answered an L2 search before, so the
           workspaces both metrics share exist already.
Every timing is the median (and min - max) of `--reps` calls on the host clock around the call, after a warm-up call of
each; the calls alternate (u8 ip, i8 ip, fp32 ip, u8 L2, then again), so that a drift of the box falls on all alike.
`--l2-only` times nothing but the L2 search of the u8 handle, in a process of its own: the figure to hold against the
same calls on another build of the library.
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


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--l2-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_ip_bytes_line.json"))
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("needs a GPU: there is no CPU path to time")
    rng = np.random.default_rng(100)
    base = rng.integers(0, 256, size=(args.n, args.dim), dtype=np.uint8)
    qs = rng.integers(0, 256, size=(args.nq, args.dim), dtype=np.uint8)
    out = dict(n=args.n, dim=args.dim, nq=args.nq, top_k=args.topk, reps=args.reps)
    if args.l2_only:
        with api.FlatIndexU8(base) as f:
            f.search(qs, args.topk)
            out["search_l2_u8_call_ms"] = spread([clock(lambda: f.search(qs, args.topk))[1] for _ in range(args.reps)])
        print(json.dumps(out))
        return

    signed = (base ^ 0x80).view(np.int8)           # the same bytes minus 128: what the u8 handle stores
    sq = (qs ^ 0x80).view(np.int8)
    wq = qs.astype(np.float32)
    u8, i8, f32 = api.FlatIndexU8(base), api.FlatIndexI8(signed), api.FlatIndex(base.astype(np.float32))
    calls = {"search_ip_u8": lambda: u8.search_ip(qs, args.topk), "search_ip_i8": lambda: i8.search_ip(sq, args.topk),
             "search_ip_fp32": lambda: f32.search_ip(wq, args.topk), "search_l2_u8": lambda: u8.search(qs, args.topk)}
    answers = {name: call() for name, call in calls.items()}      # warm-up: workspaces, code objects, the row sums
    ms = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            ms[name].append(clock(call)[1])
    for name in calls:
        out[name + "_call_ms"] = spread(ms[name])
    out["search_ip_u8_equals_fp32_over_widened"] = same(answers["search_ip_u8"], answers["search_ip_fp32"])
    with api.FlatIndex(signed.astype(np.float32)) as w:
        out["search_ip_i8_equals_fp32_over_widened"] = same(answers["search_ip_i8"], w.search_ip(sq.astype(np.float32), args.topk))
    Dp8, Dp32 = (args.dim + 31) // 32 * 32, (args.dim + 3) // 4 * 4
    out["device_bytes"] = dict(u8=args.n * Dp8 + 4 * args.n, u8_after_first_ip=args.n * Dp8 + 8 * args.n,
                               i8=args.n * Dp8 + 4 * args.n, fp32=4 * args.n * Dp32)
    for h in (i8, f32):
        h.close()
    steady = out["search_ip_u8_call_ms"]["median"]
    first = []
    for _ in range(args.reps):
        with api.FlatIndexU8(base) as f:
            f.search(qs, args.topk)
            first.append(clock(lambda: f.search_ip(qs, args.topk))[1])
    u8.close()
    out["first_search_ip_u8_call_ms"] = spread(first)
    out["row_sums_first_call_extra_ms"] = statistics.median(first) - steady
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
