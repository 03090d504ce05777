"""The exact-search rules of include/deltapq_amd.h restated in numpy (written from the rules, test infrastructure).

For a base vector v and a query q, both fp32 [D]: acc is fp64 and starts at +0.0; for d ascending, t = v[d] - q[d] in
fp32, s = t * t in fp32 (rounded on its own), acc += (double)s.  The distance is (float)acc.  A result list is the k
smallest keys `distance bits << 32 | id` in ascending order: (distance, id), the lowest ids first among equal distances.
"""
import numpy as np

PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def distances(base, q):
    """fp32 [n]: the distance of every row of base [n][D] to q [D]."""
    base = np.asarray(base, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    acc = np.zeros(base.shape[0], dtype=np.float64)
    for d in range(base.shape[1]):
        t = (base[:, d] - q[d]).astype(np.float32)
        s = (t * t).astype(np.float32)
        acc += s.astype(np.float64)
    return acc.astype(np.float32)


def keys(dists, ids):
    return (dists.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)


def unpack(k, top_k):
    """keys (sorted, at most top_k used) -> ids int32 [top_k], dists fp32 [top_k], padded with -1 / +inf."""
    ids = np.full(top_k, -1, dtype=np.int32)
    dists = np.full(top_k, np.inf, dtype=np.float32)
    k = k[:top_k]
    ids[:len(k)] = (k & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
    dists[:len(k)] = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return ids, dists


def search(base, queries, top_k, id_offset=0):
    """ids int32 [nq][top_k], dists fp32 [nq][top_k]."""
    out_i, out_d = [], []
    rows = np.arange(len(base), dtype=np.int64) + id_offset
    for q in np.asarray(queries, dtype=np.float32):
        i, d = unpack(np.sort(keys(distances(base, q), rows)), top_k)
        out_i.append(i)
        out_d.append(d)
    return np.stack(out_i), np.stack(out_d)


def rerank(base, queries, cand, top_k, id_offset=0, id_map=None):
    """The rules of dpq_flat_rerank: negative candidates are padding; without a map a candidate is row + id_offset,
    with one it is a DFS position (row = map[c]; for an even len(map) the candidate len(map) means the last
    position); a row named twice counts once; rows are padded with -1 / +inf."""
    base = np.asarray(base, dtype=np.float32)
    out_i, out_d = [], []
    for q, cs in zip(np.asarray(queries, dtype=np.float32), np.asarray(cand)):
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
        d = distances(base[rows], q) if len(rows) else np.zeros(0, dtype=np.float32)
        i, dd = unpack(np.sort(keys(d, rows + id_offset)), top_k)
        out_i.append(i)
        out_d.append(dd)
    return np.stack(out_i), np.stack(out_d)


def recall(found, truth, k, R):
    """(1 / (nq * k)) * sum over q of |found[q][:R] & truth[q][:k]|, negative ids ignored."""
    hits = 0
    for f, t in zip(found, truth):
        hits += len({int(x) for x in f[:R] if x >= 0} & {int(x) for x in t[:k] if x >= 0})
    return hits / (len(found) * k)
