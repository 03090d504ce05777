"""The rules of the exact filtered and range search (include/deltapq_amd.h) restated in numpy, on top of
_exact_restatement (written from the rules, test infrastructure).

A filter is a bitmap over reported ids (row + id_offset): bit i is bit (i & 31) of words[i >> 5]; an id at or beyond
n_bits is not eligible.  A filtered search is the unfiltered one over the eligible rows only, padded with -1 / +inf.
A range search returns every eligible row with d < r on fp32, each list ascending by key (distance bits << 32 | id).
"""
import numpy as np

import _exact_restatement as X


def eligible(n, id_offset, words, n_bits):
    """bool [n]: whether row r (reported id r + id_offset) is eligible; words None = no filter."""
    if words is None:
        return np.ones(n, dtype=bool)
    words = np.asarray(words, dtype=np.uint32).astype(np.int64)
    out = np.zeros(n, dtype=bool)
    i = np.arange(n, dtype=np.int64) + id_offset
    in_map = i < n_bits
    out[in_map] = ((words[i[in_map] >> 5] >> (i[in_map] & 31)) & 1).astype(bool)
    return out


def all_distances(base, queries):
    """fp32 [nq][n]: X.distances of every query, for the tests that answer many searches over one base."""
    base = np.asarray(base, dtype=np.float32)
    return np.stack([X.distances(base, q) for q in np.asarray(queries, dtype=np.float32)])


def search_filtered(base, queries, top_k, words, n_bits, id_offset=0, dist=None):
    """ids int32 [nq][top_k], dists fp32 [nq][top_k]: X.search over the eligible rows only.  dist: all_distances(base,
    queries), when the caller has it already (a row's distance does not depend on the other rows)."""
    base = np.asarray(base, dtype=np.float32)
    rows = np.flatnonzero(eligible(len(base), id_offset, words, n_bits))
    out_i, out_d = [], []
    for qi, q in enumerate(np.asarray(queries, dtype=np.float32)):
        if dist is not None:
            d = dist[qi][rows]
        else:
            d = X.distances(base[rows], q) if len(rows) else np.zeros(0, dtype=np.float32)
        i, dd = X.unpack(np.sort(X.keys(d, rows + id_offset)), top_k)
        out_i.append(i)
        out_d.append(dd)
    return np.stack(out_i), np.stack(out_d)


def range_search(base, queries, radii, words=None, n_bits=0, id_offset=0, dist=None):
    """(lims int64 [nq + 1], ids int32, dists fp32): per query every eligible row with d < r (fp32 compare; a radius
    <= 0 gives nothing, +inf everything), ascending by key.  dist: as in search_filtered."""
    base = np.asarray(base, dtype=np.float32)
    queries = np.asarray(queries, dtype=np.float32)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(queries),))
    rows = np.flatnonzero(eligible(len(base), id_offset, words, n_bits))
    lims, ids, dists = [0], [], []
    for qi, (q, r) in enumerate(zip(queries, radii)):
        assert not np.isnan(r)
        if dist is not None:
            d = dist[qi][rows]
        else:
            d = X.distances(base[rows], q) if len(rows) else np.zeros(0, dtype=np.float32)
        keep = d < r if r > 0 else np.zeros(len(d), dtype=bool)
        k = np.sort(X.keys(d[keep], rows[keep] + id_offset))
        i, dd = X.unpack(k, len(k))
        ids.append(i)
        dists.append(dd)
        lims.append(lims[-1] + len(k))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(ids).astype(np.int32) if ids else np.zeros(0, np.int32),
            np.concatenate(dists).astype(np.float32) if dists else np.zeros(0, np.float32))


def bitmap_to_dfs(words, n_bits, vec_id):
    """uint32 [(N + 1 + 31) // 32]: for DFS position p with reported id r (r = p, except that the last position of an even
    N is reported as N), bit r = bit vec_id[p] of the input, 0 when vec_id[p] >= n_bits."""
    n = len(vec_id)
    out = np.zeros((n + 1 + 31) // 32, dtype=np.uint32)
    for p, v in enumerate(vec_id):
        v = int(v)
        if v < n_bits and (int(words[v >> 5]) >> (v & 31)) & 1:
            r = n if (n % 2 == 0 and p == n - 1) else p
            out[r >> 5] |= np.uint32(1 << (r & 31))
    return out


def range_recall(found, truth):
    """(recall, precision) summed over queries; an id counts once per query, negative ids are ignored, 0 / 0 = 1."""
    (fl, fi), (tl, ti) = found[:2], truth[:2]
    hits = n_f = n_t = 0
    for q in range(len(fl) - 1):
        f = {int(x) for x in fi[fl[q]:fl[q + 1]] if x >= 0}
        t = {int(x) for x in ti[tl[q]:tl[q + 1]] if x >= 0}
        hits += len(f & t)
        n_f += len(f)
        n_t += len(t)
    return (hits / n_t if n_t else 1.0), (hits / n_f if n_f else 1.0)
