"""tests/_kmeanspp_restatement.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (helper, not collected).

CPU restatement, in numpy, of the k-means++ start, the leaf-ordered potential and the restart rule of
dpq_train_codebook (include/deltapq_amd.h), built on tests/_kmeans_restatement.py.  These rules are
this build's own, and the GPU is compared with this file bit for bit.

  rng        per sub-space m: s = seed + m * 0xD6E8FEB86659FD93; next(): s += 0x9E3779B97F4A7C15, splitmix64 finaliser
  centre 0   sub-vector next() % n; w_i = the fp32 assignment distance of sub-vector i to it
  leaves     256 consecutive vectors; S_l the fp64 sum from +0.0 of w_i in ascending i, one add after the other
             (a cumulative sum); T the cumulative sum of S; total the last T
  draw       total == 0: the smallest index that is no centre yet.  Otherwise u = (z >> 11) * 2**-53, r = u * total,
             the first leaf with T_l > r (none: the last with S_l > 0), r' = r - T_{l-1}, the first i of the leaf whose
             running sum exceeds r' (none: the leaf's last i with w_i > 0)
  update     w_i = d if d < w_i else w_i, d the distance to the new centre
  potential  total over the final w (seeding) or over the winning distances of one assignment (a codebook)
  restarts   run r is a complete run with seed + r; per sub-space the lowest potential wins, ties to the lowest r
"""
import numpy as np

import _kmeans_restatement as R

LEAF = 256
_MASK = (1 << 64) - 1


class Rng:
    def __init__(self, seed, m=0):
        self.s = (seed + m * 0xD6E8FEB86659FD93) & _MASK

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _MASK
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
        return z ^ (z >> 31)


def leaf_running(w):
    """float64 [L][256]: per leaf the running in-order sums of the fp32 weights (a short leaf padded with +0.0, which
    leaves a non-negative running sum as it is)."""
    n = len(w)
    L = -(-n // LEAF)
    p = np.zeros(L * LEAF, dtype=np.float64)
    p[:n] = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.cumsum(p.reshape(L, LEAF), axis=1)


def leaf_totals(w):
    """(S float64 [L], T float64 [L]) of fp32 weights."""
    S = leaf_running(w)[:, -1].copy()
    return S, np.cumsum(S)


def potential_of_weights(w):
    return float(leaf_totals(w)[1][-1])


def distance_to(sub, row):
    return R.assign(sub, sub[row:row + 1])[1]


def draw(w, z, centres):
    """(chosen index, what decided: "zero", "walk", "leaf-fallback", "row-fallback" joined by +)."""
    n = len(w)
    S, T = leaf_totals(w)
    total = T[-1]
    if total == 0.0:
        taken = set(centres)
        return next(i for i in range(n) if i not in taken), "zero"
    u = np.float64(z >> 11) * np.float64(2.0 ** -53)
    r = u * total
    how = []
    above = np.flatnonzero(T > r)
    if len(above):
        leaf = int(above[0])
    else:
        leaf = int(np.flatnonzero(S > 0.0)[-1])
        how.append("leaf-fallback")
    rp = r - (T[leaf - 1] if leaf else np.float64(0.0))
    lo = leaf * LEAF
    cnt = min(LEAF, n - lo)
    t = leaf_running(w[lo:lo + cnt])[0][:cnt]
    over = np.flatnonzero(t > rp)
    if len(over):
        i = int(over[0])
        how.append("walk")
    else:
        i = int(np.flatnonzero(w[lo:lo + cnt] > 0)[-1])
        how.append("row-fallback")
    return lo + i, "+".join(how)


def seed_subspace(sub, K, seed, m=0):
    """(rows list [K], final weights float32 [n], potential, how list [K - 1]) of one sub-space."""
    n = len(sub)
    rng = Rng(seed, m)
    rows = [rng.next() % n]
    w = distance_to(sub, rows[0])
    how = []
    for _ in range(1, K):
        i, h = draw(w, rng.next(), rows)
        rows.append(i)
        how.append(h)
        d = distance_to(sub, i)
        w = np.where(d < w, d, w).astype(np.float32)
    return rows, w, potential_of_weights(w), how


def kmeanspp_seed(vectors, M, K, seed=0):
    """(codebook float32 [M][K][Ds], potential float64 [M], info) -- info carries rows and how per sub-space."""
    subs = R.split(vectors, M)
    out = [seed_subspace(s, K, seed, m) for m, s in enumerate(subs)]
    cb = np.stack([s[o[0]] for s, o in zip(subs, out)]).astype(np.float32)
    return cb, np.array([o[2] for o in out], dtype=np.float64), dict(rows=[o[0] for o in out], how=[o[3] for o in out])


def potential(vectors, codebook):
    """float64 [M]: the leaf-ordered sum of the winning distances of one assignment."""
    cb = np.asarray(codebook, dtype=np.float32)
    return np.array([potential_of_weights(R.assign(s, cb[m])[1]) for m, s in enumerate(R.split(vectors, len(cb)))],
                    dtype=np.float64)


def train(vectors, M, K, max_iters=25, seed=0, init=None, start="rows", restarts=1):
    """(codebook, stats) by the restart rule; stats also carries `winner` (the run each sub-space kept) and `runs`."""
    assert start in ("rows", "kmeans++") and not (start == "kmeans++" and init is not None)
    runs = []
    for r in range(max(1, restarts)):
        s = (seed + r) & _MASK
        first = kmeanspp_seed(vectors, M, K, s)[0] if start == "kmeans++" else init
        cb, st = R.train(vectors, M, K, max_iters, s, first)
        runs.append((cb, st, potential(vectors, cb)))
    pots = np.stack([p for _, _, p in runs])                 # [runs][M]
    winner = pots.argmin(0)                                  # argmin returns the first minimum: the lowest r
    cb = np.stack([runs[winner[m]][0][m] for m in range(M)])
    stats = dict(iters_run=max(st["iters_run"] for _, st, _ in runs),
                 converged=int(all(st["converged"] for _, st, _ in runs)),
                 reseeded=sum(st["reseeded"] for _, st, _ in runs),
                 distortion=runs[0][1]["distortion"], winner=winner.tolist(), runs=runs)
    return cb, stats
