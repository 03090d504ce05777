"""Developer simulation (CPU, numpy): survivors per query of the scan's lower-bound filter at M = 8 under four splits of
the saturation budget -- uniform (SAT_BUDGET / 8 each), water-filled per query (a unit at a time to the sub-space with the most
centroids still above its saturation), the rule as built (proportional to the 32nd-largest entry of each row, capped at
QT + 1, the capped rows' surplus split again: filter_saturations in dpq_kernels.hip, restated in
tests/_filter_saturation.py) and no saturation at all -- at several QT, one filter level, threshold = the distance at a given
rank.  Bench workload: the recipe of scripts/sim_filter_nibbles.py.
  python scripts/sim_filter_saturation.py [N = 1000000] [queries = 24]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from deltapq_amd import synth
from oracle import pq_encode_oracle

N, M, K = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000, 8, 256
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 24
RANKS = [800, 200]
QTS = [64, 72, 80, 88]
XMAX, XU, RANK = 7, 1, 32
cache = "/tmp/sim_filter_%d.npz" % N
if os.path.exists(cache):
    z = np.load(cache)
    cb, codes, queries = z["cb"], z["codes"], z["queries"]
else:
    base = synth.make_clustered_vectors(N, 128, seed=100, n_clusters=20000, spread=12.0, centre_seed=7)
    queries = synth.make_clustered_vectors(48, 128, seed=101, n_clusters=20000, spread=12.0, centre_seed=7)
    cb = synth.kmeans_codebook(base, M, 256, iters=6, seed=102)
    codes = pq_encode_oracle.encode_pq(base, cb)
    del base
    np.savez(cache, cb=cb, codes=codes, queries=queries)
Ds = 128 // M


def budget(qt):
    return 255 - (127 - (qt + 1)) - XMAX * XU


def water_filled(x, qt):
    """x int [M][K] clipped to qt + 1: hand the budget out a unit at a time to the row with the most entries above its saturation."""
    sat = np.zeros(M, dtype=np.int64)
    above = np.array([[np.count_nonzero(x[m] > s) for s in range(qt + 2)] for m in range(M)])    # [m][s]: entries > s
    for _ in range(budget(qt)):
        gain = np.where(sat <= qt, above[np.arange(M), np.minimum(sat, qt + 1)], -1)
        m = int(np.argmax(gain))
        if gain[m] <= 0:
            break
        sat[m] += 1
    return sat


def as_built(x, qt):
    """Proportional to the RANK-th largest entry, capped at qt + 1 (tests/_filter_saturation.saturations_of_stats)."""
    cap, bud = qt + 1, budget(qt)
    stat = [int(np.sort(x[m])[::-1][RANK - 1]) for m in range(M)]
    if not any(stat):
        return np.full(M, bud // M)
    sat, open_, rem = [0] * M, list(range(M)), bud
    while open_:
        S = sum(stat[m] for m in open_)
        if S == 0:
            for m in open_:
                sat[m] = min(rem // len(open_), cap)
            break
        capped = [m for m in open_ if rem * stat[m] >= cap * S]
        if not capped:
            for m in open_:
                sat[m] = rem * stat[m] // S
            break
        for m in capped:
            sat[m] = cap
        rem -= cap * len(capped)
        open_ = [m for m in open_ if m not in capped]
    left = bud - sum(sat)
    for m in range(M):
        if left > 0 and sat[m] < cap:
            sat[m] += 1
            left -= 1
    return np.array(sat)


def survivors(e, sat, qt):
    sq = np.minimum(e, sat[:, None])[np.arange(M)[None, :], codes].sum(axis=1)
    return int((sq <= qt).sum())


names = ["uniform", "water-filled", "as built", "none"]
res = {(r, qt): [] for r in RANKS for qt in QTS}
for qi in range(min(NQ, len(queries))):
    q = queries[qi].reshape(M, Ds)
    T = ((cb - q[:, None, :]) ** 2).sum(axis=2).astype(np.float64)
    mn = T.min(axis=1)
    d = T[np.arange(M)[None, :], codes].sum(axis=1)
    for rank in RANKS:
        tau = np.partition(d, rank - 1)[rank - 1]
        for qt in QTS:
            s = qt / (tau * (1 + 2.0 ** -20) - mn.sum())
            e = np.floor((T - mn[:, None]) * s).astype(np.int64)
            x = np.minimum(e, qt + 1)
            res[(rank, qt)].append([survivors(e, np.full(M, budget(qt) // M), qt), survivors(e, water_filled(x, qt), qt),
                                    survivors(e, as_built(x, qt), qt), survivors(e, np.full(M, 1 << 30), qt)])
print("N = %d, %d queries; survivors per query, mean (max)" % (N, min(NQ, len(queries))))
print("%-6s %-4s " % ("rank", "QT") + " ".join("%-16s" % n for n in names))
for rank in RANKS:
    for qt in QTS:
        r = np.array(res[(rank, qt)], dtype=np.float64)
        print("%-6d %-4d " % (rank, qt) + " ".join("%-16s" % ("%.0f (%.0f)" % (a, b)) for a, b in zip(r.mean(axis=0), r.max(axis=0))))
