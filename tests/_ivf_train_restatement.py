"""The rules of the IVF training (include/deltapq_amd.h "IVF training"), restated in numpy for tests/test_ivf_train.py.
No tests in here, and nothing but numpy.

  distance  tests/_exact_restatement.py: fp32 difference, fp32 square, fp64 sum in dimension order, rounded once
  assign    tests/_ivf_restatement.py's assign (the lowest list at a tie), and the winning distance to that list
  start     the caller's centroids, or tests/_kmeans_restatement.py's seeded_rows(n, nlist, seed)
  stop, update, empty   tests/_kmeans_restatement.py's update on one sub-space with K = nlist, Ds = D
  distortion  the fp64 sum of the winning distances (numpy's order: the GPU's may differ by n * 2^-52 relative)
"""
import numpy as np

import _exact_restatement as E
import _ivf_restatement as I
import _kmeans_restatement as K

seeded_rows = K.seeded_rows
update = K.update


def assign(vectors, centroids):
    """(labels int64 [n], winning distances float32 [n])."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    c = np.ascontiguousarray(centroids, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        lab = I.assign(v, c).astype(np.int64)
        win = np.empty(len(v), dtype=np.float32)
        for l in np.unique(lab):
            members = np.flatnonzero(lab == l)
            # v - c here, c - v in the header: the fp32 difference changes its sign with the order of its operands and
            # its square does not (_ivf_restatement.assign relies on the same)
            win[members] = E.distances(v[members], c[l])
    return lab, win


def distortion_bound(n, value):
    """What two fp64 sums of n non-negative terms in different orders may differ by."""
    return n * 2.0 ** -52 * abs(value)


def train(vectors, nlist, max_iters=25, seed=0, init=None):
    """(centroids float32 [nlist][D], stats dict: iters_run, converged, reseeded, distortion, labels)."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    n = len(v)
    if init is None:
        c = v[seeded_rows(n, nlist, seed)].copy()
    else:
        c = np.array(init, dtype=np.float32)
        assert c.shape == (nlist, v.shape[1])
    labels, distortion, reseeded, iters_run, converged = None, [], 0, 0, False
    for r in range(max_iters):
        iters_run = r + 1
        lab, win = assign(v, c)
        changed = n if labels is None else int((lab != labels).sum())
        n_empty = nlist - len(np.unique(lab))
        labels = lab
        distortion.append(float(win.astype(np.float64).sum()))
        if r > 0 and changed == 0 and n_empty == 0:
            converged = True
            break
        c, e = update(v, lab, win, c)
        reseeded += e
    return c, dict(iters_run=iters_run, converged=int(converged), reseeded=reseeded, distortion=distortion, labels=labels)
