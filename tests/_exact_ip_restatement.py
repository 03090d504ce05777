"""The exact inner-product rules of include/deltapq_amd.h restated in numpy (written from the rules, test infrastructure).

For a base vector v and a query q, both fp32 [D]: acc is fp64 and starts at +0.0; for d ascending,
acc = acc + (double)v[d] * (double)q[d] -- the product of two fp32 values is exact in fp64, so a step is one rounding.
The score is (float)acc, and -0.0 is reported and ordered as +0.0.  A result list is the k smallest keys `hi << 32 | id`
in ascending order, with hi = (u & 0x80000000) ? u : (~u & 0x7fffffff) over the bits u of the normalised score:
(score descending, id ascending).  Padding is -1 / -inf.  A range list holds the rows with score > threshold, strictly.
"""
import numpy as np

PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def scores(base, q):
    """fp32 [n]: the score of every row of base [n][D] against q [D]."""
    base = np.asarray(base, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    acc = np.zeros(base.shape[0], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(base.shape[1]):
            acc = acc + base[:, d].astype(np.float64) * np.float64(q[d])
        s = acc.astype(np.float32)
    return s + np.float32(0)       # -0.0 + +0.0 = +0.0; every other value is unchanged


def word(u):
    """Score bits uint32 -> the high word of a key; its own inverse.  -0.0 is read as +0.0."""
    u = np.asarray(u, dtype=np.uint32)
    u = np.where(u == np.uint32(0x80000000), np.uint32(0), u)
    return np.where(u & np.uint32(0x80000000), u, ~u & np.uint32(0x7FFFFFFF)).astype(np.uint32)


def keys(s, ids):
    w = word(np.asarray(s, dtype=np.float32).view(np.uint32))
    return (w.astype(np.uint64) << np.uint64(32)) | np.asarray(ids).astype(np.uint64)


def unpack(k, top_k):
    """keys (sorted, at most top_k used) -> ids int32 [top_k], scores fp32 [top_k], padded with -1 / -inf."""
    ids = np.full(top_k, -1, dtype=np.int32)
    s = np.full(top_k, -np.inf, dtype=np.float32)
    k = k[:top_k]
    ids[:len(k)] = (k & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
    s[:len(k)] = word((k >> np.uint64(32)).astype(np.uint32)).view(np.float32)
    return ids, s


def all_scores(base, queries):
    """fp32 [nq][n]; computed once and handed to the functions below by the tests that share a data set."""
    return np.stack([scores(base, q) for q in np.asarray(queries, dtype=np.float32)])


def search(base, queries, top_k, id_offset=0, allowed=None, table=None):
    """ids int32 [nq][top_k], scores fp32 [nq][top_k].  allowed: bool [n], the rows a filter lets through."""
    table = all_scores(base, queries) if table is None else table
    rows = np.arange(table.shape[1], dtype=np.int64)
    if allowed is not None:
        rows = rows[np.asarray(allowed, dtype=bool)]
    out = [unpack(np.sort(keys(s[rows], rows + id_offset)), top_k) for s in table]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_search(base, queries, thresholds, id_offset=0, allowed=None, table=None):
    """(lims int64 [nq + 1], ids int32, scores fp32): per query the rows with score > threshold, by key."""
    table = all_scores(base, queries) if table is None else table
    thr = np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (table.shape[0],))
    rows = np.arange(table.shape[1], dtype=np.int64)
    if allowed is not None:
        rows = rows[np.asarray(allowed, dtype=bool)]
    lims, ids, out = [0], [], []
    for s, t in zip(table, thr):
        keep = s[rows] > t
        i, sc = unpack(np.sort(keys(s[rows][keep], rows[keep] + id_offset)), int(keep.sum()))
        ids.append(i)
        out.append(sc)
        lims.append(lims[-1] + len(i))
    return np.array(lims, dtype=np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(out).astype(np.float32)


def rerank(base, queries, cand, top_k, id_offset=0, id_map=None):
    """The rules of dpq_flat_rerank_ip: negative candidates are padding; without a map a candidate is row + id_offset,
    with one it is a DFS position (row = map[c]; for an even len(map) the candidate len(map) means the last position); a
    row named twice counts once; rows are padded with -1 / -inf."""
    base = np.asarray(base, dtype=np.float32)
    out_i, out_s = [], []
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
        s = scores(base[rows], q) if len(rows) else np.zeros(0, dtype=np.float32)
        i, ss = unpack(np.sort(keys(s, rows + id_offset)), top_k)
        out_i.append(i)
        out_s.append(ss)
    return np.stack(out_i), np.stack(out_s)


def merge(ids, s):
    """ids / scores [n_lists][nq][k] -> [nq][k]: negative ids are padding, repeated rows are kept."""
    ids, s = np.asarray(ids, dtype=np.int32), np.asarray(s, dtype=np.float32)
    n_lists, nq, k = ids.shape
    out = []
    for q in range(nq):
        i, sc = ids[:, q, :].ravel(), s[:, q, :].ravel()
        out.append(unpack(np.sort(keys(sc[i >= 0], i[i >= 0].astype(np.int64))), k))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def recall(found, truth, k, R):
    """(1 / (nq * k)) * sum over q of |found[q][:R] & truth[q][:k]|, negative ids ignored."""
    hits = 0
    for f, t in zip(found, truth):
        hits += len({int(x) for x in f[:R] if x >= 0} & {int(x) for x in t[:k] if x >= 0})
    return hits / (len(found) * k)
