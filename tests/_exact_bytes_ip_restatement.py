"""The byte rules of "exact inner product over byte vectors; signed int8 storage" (include/deltapq_amd.h) restated in
numpy (test infrastructure): a score is the int64 dot product of the bytes, a distance the int64 sum of their squared
differences, each converted to fp32, round to nearest even (np.float32 of an int64).  The rows and the queries are uint8
(0..255) or int8 (-128..127), never mixed.  Keys, order, padding and the candidate rules are those of
_exact_ip_restatement (metric "ip") and _exact_restatement (metric "l2"), whose word / keys / unpack are used as they are.
"""
import numpy as np

import _exact_ip_restatement as XI
import _exact_restatement as X


def _same_kind(base, queries):
    assert base.dtype == queries.dtype and base.dtype in (np.uint8, np.int8), (base.dtype, queries.dtype)


def table(base, queries, metric):
    """fp32 [nq][n]: the score ("ip") or the distance ("l2") of every query against every row.  The distances come from
    |v|^2 + |q|^2 - 2 v.q in int64, which is the sum of the squared differences exactly (test_restatement checks it)."""
    _same_kind(base, queries)
    b, q = base.astype(np.int64), queries.astype(np.int64)
    dot = q @ b.T
    if metric == "ip":
        return dot.astype(np.float32)
    assert metric == "l2"
    return ((q * q).sum(-1)[:, None] + (b * b).sum(-1)[None, :] - 2 * dot).astype(np.float32)


def _pack(metric):
    return (XI.keys, XI.unpack) if metric == "ip" else (X.keys, X.unpack)


def _rows(n, allowed):
    rows = np.arange(n, dtype=np.int64)
    return rows if allowed is None else rows[np.asarray(allowed, dtype=bool)]


def search(tab, top_k, metric, id_offset=0, allowed=None):
    """ids int32 [nq][top_k], values fp32 [nq][top_k] from a table; allowed: bool [n], the rows a filter lets through."""
    keys, unpack = _pack(metric)
    rows = _rows(tab.shape[1], allowed)
    out = [unpack(np.sort(keys(t[rows], rows + id_offset)), top_k) for t in tab]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_search(tab, bounds, metric, id_offset=0, allowed=None):
    """(lims int64 [nq + 1], ids int32, values fp32): "ip" the rows with score > threshold, "l2" those with distance <
    radius (a radius <= 0 keeps nothing), strictly, each list by key."""
    keys, unpack = _pack(metric)
    bounds = np.broadcast_to(np.asarray(bounds, dtype=np.float32), (tab.shape[0],))
    rows = _rows(tab.shape[1], allowed)
    lims, ids, vals = [0], [], []
    for t, r in zip(tab, bounds):
        assert not np.isnan(r)
        keep = t[rows] > r if metric == "ip" else (t[rows] < r if r > 0 else np.zeros(len(rows), dtype=bool))
        i, v = unpack(np.sort(keys(t[rows][keep], rows[keep] + id_offset)), int(keep.sum()))
        ids.append(i)
        vals.append(v)
        lims.append(lims[-1] + len(i))
    return np.array(lims, dtype=np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(vals).astype(np.float32)


def rerank(base, queries, cand, top_k, metric, id_offset=0, id_map=None):
    """The candidate rules of dpq_flat_rerank*: negative candidates are padding; without a map a candidate is row +
    id_offset, with one it is a DFS position (row = map[c]; for an even len(map) the candidate len(map) means the last
    position); a row named twice counts once; rows are padded."""
    keys, unpack = _pack(metric)
    out = []
    for q, cs in zip(queries, np.asarray(cand)):
        cs = cs[cs >= 0].astype(np.int64)
        if id_map is not None:
            n_map = len(id_map)
            if n_map % 2 == 0:
                cs = np.where(cs == n_map, n_map - 1, cs)
            rows = np.asarray(id_map, dtype=np.int64)[cs]
        else:
            rows = cs - id_offset
        rows = np.unique(rows)
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < len(base))
        t = table(base[rows], q[None, :], metric)[0] if len(rows) else np.zeros(0, dtype=np.float32)
        out.append(unpack(np.sort(keys(t, rows + id_offset)), top_k))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
