"""The rules of the candidate search (include/deltapq_amd.h "candidate search"), restated in numpy for
tests/test_candidate_search.py.  No tests in here, and nothing but numpy.

Ids: what a candidate is to a handle, from (id_base, n_local, n_total, even_rule).  Distances: either rule of
tests/_tables_restatement.py over the candidates' codes.  Answer: keys `distance bits << 32 | id` ascending, a key once,
padded with -1 / +inf.
"""
import numpy as np

import _tables_restatement as T

LOCAL, SKIP, NONE = 1, 0, -1


def classify(ids, id_base, n_local, n_total, even_rule):
    """(cls int [..], local int64 [..]): LOCAL with the local position of the node, SKIP for padding (negative) and for a
    node of the index another handle holds, NONE for an id that names no node of the index.  even_rule (a DTC handle): for
    an even n_total the id n_total names position n_total - 1 and n_total - 1 names nothing."""
    ids = np.asarray(ids, dtype=np.int64)
    pos = ids.copy()
    none = np.zeros(ids.shape, dtype=bool)
    if even_rule and n_total % 2 == 0:
        none |= ids == n_total - 1
        pos[ids == n_total] = n_total - 1
    none |= pos >= n_total
    none &= ids >= 0
    local = pos - id_base
    here = (ids >= 0) & ~none & (local >= 0) & (local < n_local)
    cls = np.where(none, NONE, np.where(here, LOCAL, SKIP))
    return cls, np.where(here, local, -1)


def distances(table, codes, plain):
    """float32 [n]: the distance of every code under one table [M][K], by the handle's rule."""
    return T.distances_plain(table, codes) if plain else T.distances_dtc(table, codes)


def candidate_distances(d, cand, id_base=0, n_local=None, n_total=None, even_rule=True):
    """float32 [n_cand]: d[local position] of every candidate of one query, a quiet NaN where it is not LOCAL.  d holds
    the handle's distances by local position.  Raises ValueError where a candidate names no node."""
    n_local = len(d) if n_local is None else n_local
    n_total = id_base + n_local if n_total is None else n_total
    cls, local = classify(cand, id_base, n_local, n_total, even_rule)
    if np.any(cls == NONE):
        raise ValueError("a candidate names no node of the index")
    out = np.full(len(cls), np.nan, dtype=np.float32)
    out[cls == LOCAL] = np.asarray(d, dtype=np.float32)[local[cls == LOCAL]]
    return out


def search_row(d, cand, top_k, **ids):
    """(ids int32 [top_k], dists float32 [top_k]) of one query: the valid candidates by (distance bits, id), each key
    once, padded with -1 / +inf."""
    cand = np.asarray(cand, dtype=np.int64)
    dist = candidate_distances(d, cand, **ids)
    ok = ~np.isnan(dist)
    keys = (dist[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand[ok].astype(np.uint64)
    keys = np.unique(keys)[:top_k]                        # sorted, repeats dropped
    out_i = np.full(top_k, -1, dtype=np.int32)
    out_d = np.full(top_k, np.inf, dtype=np.float32)
    out_i[:len(keys)] = (keys & np.uint64(0xffffffff)).astype(np.int32)
    out_d[:len(keys)] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return out_i, out_d
