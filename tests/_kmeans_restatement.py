"""tests/_kmeans_restatement.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (helper, not collected).

CPU restatement, in numpy, of the codebook learning rules of dpq_train_codebook (include/deltapq_amd.h,
DESIGN.md 5.9).  No reference semantics (cv::kmeans): the rules are this build's own, and the GPU is compared
with this file bit for bit.

  start    the caller's codebook, or K rows drawn by the splitmix64 partial shuffle below, the same rows for
           every sub-space
  assign   oracle/pq_encode_oracle.py's arithmetic (fp32, separately rounded subtract / multiply / add,
           dimensions in order) and its selection (start at FLT_MAX, strict `<`: the first minimum wins, and the label
           is 0 when no distance is below FLT_MAX); the winning distance is the computed distance to that label,
           +inf when every distance overflows
  stop     after an assignment (not the first) that changes no label and leaves no cluster empty
  update   fp64 sum, starting from +0.0, of the members' fp32 values in ascending vector index, one add after the
           other (a cumulative sum over the members in that order), / float64(count), rounded once to fp32
  empty    the j-th empty cluster in ascending k takes the j-th vector ranked by (winning distance descending,
           vector index ascending); the donor stays in its old cluster's mean of this round
"""
import numpy as np

from oracle import pq_encode_oracle as E     # the encoder's selection rule: one statement of it, not two

_MASK = (1 << 64) - 1


def seeded_rows(n, K, seed):
    p = list(range(n))
    s = seed & _MASK
    for i in range(K):
        s = (s + 0x9E3779B97F4A7C15) & _MASK
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
        z ^= z >> 31
        j = i + z % (n - i)
        p[i], p[j] = p[j], p[i]
    return p[:K]


def split(vectors, M):
    """[M] arrays [n][Ds], Ds = ceil(D / M), short vectors zero padded (pq.cpp:114-123)."""
    v = np.asarray(vectors, dtype=np.float32)
    n, D = v.shape
    Ds = -(-D // M)
    padded = np.zeros((n, M * Ds), dtype=np.float32)
    padded[:, :D] = v
    return [np.ascontiguousarray(padded[:, m * Ds:(m + 1) * Ds]) for m in range(M)]


def assign(sub, c):
    """labels int64 [n], winning distances float32 [n].  The label is the encoder's own selection
    (oracle/pq_encode_oracle.py: start at FLT_MAX, strict `<`, so 0 when nothing is below FLT_MAX), and the winning
    distance is the computed distance to that label: +inf when every distance overflows."""
    n, Ds = sub.shape
    dist = np.zeros((n, len(c)), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for d in range(Ds):
            diff = (sub[:, d:d + 1] - c[:, d][None, :]).astype(np.float32)
            dist = (dist + (diff * diff).astype(np.float32)).astype(np.float32)
    lab = E.select(dist)
    return lab, dist[np.arange(n), lab]


def update(sub, lab, win, c):
    """The codebook after one update + repair; returns (codebook, number of empty clusters)."""
    n, Ds = sub.shape
    K = len(c)
    c = c.copy()
    order = np.argsort(lab, kind="stable")    # members of a cluster in ascending vector index
    counts = np.bincount(lab, minlength=K)
    x = sub[order].astype(np.float64)
    at = 0
    for k in range(K):
        if counts[k]:
            # one add after the other, starting from +0.0 (a lone member -0.0 has the mean +0.0)
            total = np.cumsum(np.concatenate([np.zeros((1, Ds)), x[at:at + counts[k]]]), axis=0)[-1]
            c[k] = (total / np.float64(counts[k])).astype(np.float32)
        at += counts[k]
    empty = np.flatnonzero(counts == 0)
    if len(empty):
        rank = np.lexsort((np.arange(n), -win.astype(np.float64)))   # distance descending, then index ascending
        for j, k in enumerate(empty):
            c[k] = sub[rank[j]]
    return c, len(empty)


def train(vectors, M, K, max_iters=25, seed=0, init=None):
    """(codebook float32 [M][K][Ds], stats) -- stats also carries the last round's labels per sub-space, and per
    round the winning distances its distortion sums (`wins`, float32 [M][n]) and the sub-spaces still active after
    its stop rule (`active`)."""
    subs = split(vectors, M)
    n, Ds = subs[0].shape
    if init is None:
        rows = seeded_rows(n, K, seed)
        cb = np.stack([s[rows] for s in subs]).astype(np.float32)
    else:
        cb = np.array(init, dtype=np.float32)
        assert cb.shape == (M, K, Ds)
    labels = [None] * M
    wins = [None] * M
    sums = [0.0] * M
    active = [True] * M
    distortion, reseeded, iters_run, converged = [], 0, 0, False
    win_trace, active_trace = [], []
    for r in range(max_iters):
        iters_run = r + 1
        todo = []
        for m in range(M):
            if not active[m]:
                continue
            lab, win = assign(subs[m], cb[m])
            changed = n if labels[m] is None else int((lab != labels[m]).sum())
            n_empty = K - len(np.unique(lab))
            labels[m] = lab
            wins[m] = win
            sums[m] = float(win.astype(np.float64).sum())
            if r > 0 and changed == 0 and n_empty == 0:
                active[m] = False
            else:
                todo.append((m, lab, win))
        distortion.append(float(sum(sums)))
        win_trace.append(np.stack(wins))
        active_trace.append(list(active))
        if not any(active):
            converged = True
            break
        for m, lab, win in todo:
            cb[m], e = update(subs[m], lab, win, cb[m])
            reseeded += e
    return cb, dict(iters_run=iters_run, converged=int(converged), reseeded=reseeded, distortion=distortion,
                    labels=np.stack(labels, axis=1), wins=win_trace, active=active_trace)
