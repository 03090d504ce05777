"""The rules of the IVF search (include/deltapq_amd.h "IVF search"), restated in numpy for tests/test_ivf_search.py.  No
tests in here, and nothing but numpy.

Lists: from labels over a handle's local nodes, holding REPORTED ids (global DFS positions, the even-N rule applied),
ascending inside a list.  Probes: the nprobe nearest centroids by (exact L2 distance, list number), over
tests/_exact_restatement.py.  Answer: tests/_candidates_restatement.py's search_row over the union of the probed lists.
"""
import numpy as np

import _candidates_restatement as C
import _exact_restatement as E


def reported_ids(node_lo, n_local, n_total=None, even_rule=True):
    """int64 [n_local]: the id a search reports for local node l (position node_lo + l)."""
    n_total = node_lo + n_local if n_total is None else n_total
    pos = node_lo + np.arange(n_local, dtype=np.int64)
    if even_rule and n_total % 2 == 0:
        pos[pos == n_total - 1] = n_total
    return pos


def lists_from_labels(labels, nlist, node_lo=0, n_total=None, even_rule=True):
    """(offsets int64 [nlist + 1], ids int32 [n_assigned]): labels[l] is the list of local node l, a negative label puts
    it in no list; a label >= nlist raises ValueError."""
    labels = np.asarray(labels, dtype=np.int64)
    if np.any(labels >= nlist):
        raise ValueError("a label is >= nlist")
    rep = reported_ids(node_lo, len(labels), n_total, even_rule)
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    chunks = []
    for l in range(nlist):
        members = rep[labels == l]                        # positions ascend, and so do their ids
        chunks.append(members)
        offsets[l + 1] = offsets[l] + len(members)
    ids = np.concatenate(chunks).astype(np.int32) if chunks else np.zeros(0, dtype=np.int32)
    return offsets, ids


def probe(centroids, queries, nprobe):
    """(lists int32 [nq][nprobe], dists float32 [nq][nprobe]): by (distance bits, list number)."""
    centroids = np.asarray(centroids, dtype=np.float32)
    return E.search(centroids, np.asarray(queries, dtype=np.float32).reshape(-1, centroids.shape[1]), nprobe)


def assign(rows, centroids):
    """int32 [n]: the nearest centroid of every row, the lowest list at a tie.  One column per centroid: the fp32
    difference changes its sign with the order of its operands and its square does not, and no distance is a NaN or
    -0.0, so the first minimum of the floats is the smallest key (distance bits, list)."""
    rows = np.asarray(rows, dtype=np.float32)
    d = np.stack([E.distances(rows, c) for c in np.asarray(centroids, dtype=np.float32)], axis=1)
    return np.argmin(d, axis=1).astype(np.int32)


def union(offsets, ids, probes_row):
    """The ids of the lists one query probes: negative entries are padding, a list named twice counts once, an entry >=
    nlist raises ValueError."""
    nlist = len(offsets) - 1
    seen, out = set(), []
    for p in np.asarray(probes_row, dtype=np.int64):
        if p >= nlist:
            raise ValueError("a probe names no list")
        if p < 0 or int(p) in seen:
            continue
        seen.add(int(p))
        out.append(np.asarray(ids[offsets[p]:offsets[p + 1]], dtype=np.int64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def search_row(d, offsets, ids, probes_row, top_k, **id_rules):
    """(ids int32 [top_k], dists float32 [top_k]) of one query.  d: the handle's distances by LOCAL position; id_rules:
    id_base, n_local, n_total, even_rule of _candidates_restatement.search_row."""
    return C.search_row(d, union(offsets, ids, probes_row), top_k, **id_rules)


def search(alld, use, offsets, ids, probes, top_k, **id_rules):
    """search_row for every query q, whose distances are alld[use[q]]."""
    return [search_row(alld[u], offsets, ids, probes[q], top_k, **id_rules) for q, u in enumerate(use)]
