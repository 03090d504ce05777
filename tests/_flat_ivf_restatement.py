"""The rules of the IVF search over raw rows (include/deltapq_amd.h "IVF search over raw vectors" and "IVF search over byte
vectors"), restated in numpy for tests/test_ivf_flat*.py.  No tests in here, and nothing but numpy.

A case is a dict with base [n][D] (float32, uint8 or int8 rows), offsets and rows (lists_from_labels).  The answer of a
query is the sorted keys (distance bits << 32 | id) of the union of the lists it probes, cut at top_k and padded with
-1 / +inf.  fp32 rows: the distance is `distances`.  Byte rows: the int64 sum of (v - q)^2, cast once to float32.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def distances(rows, q):
    """float32 [n]: t = v[d] - q[d] and s = t * t rounded in fp32, summed in float64 in ascending d, cast once."""
    t = (rows - q).astype(F32)
    s = (t * t).astype(F32)
    acc = np.zeros(len(rows), dtype=F64)
    for d in range(rows.shape[1]):
        acc += s[:, d]
    return acc.astype(F32)


def distances_bytes(rows, q):
    """float32 [n]: exact in int64, one cast."""
    return ((rows.astype(np.int64) - q.astype(np.int64)) ** 2).sum(axis=1).astype(F32)


def lists_from_labels(labels, nlist):
    """(offsets int64 [nlist + 1], rows int64 [n_assigned]): the rows of a list ascend."""
    key = np.where(labels < 0, nlist, labels)
    rows = np.argsort(key, kind="stable")[:int((labels >= 0).sum())]
    return np.concatenate([[0], np.cumsum(np.bincount(key, minlength=nlist + 1)[:nlist])]).astype(np.int64), rows


def row_keys(c, q, row, id_offset=0):
    """uint64 [m], ascending: the keys of every row of the lists the probe row names, for query q.  Padding (-1) is
    skipped, a repeat counts once.  Ids are the low 32 bits of row + id_offset."""
    dist = distances if c["base"].dtype.kind == "f" else distances_bytes
    keys = [np.zeros(0, dtype=np.uint64)]
    for l in dict.fromkeys(int(p) for p in row if p >= 0):
        r = c["rows"][c["offsets"][l]:c["offsets"][l + 1]]
        d = dist(c["base"][r], q)
        keys.append((d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (r + id_offset).astype(np.uint64))
    return np.sort(np.concatenate(keys))


def cut(keys, top_k):
    """(ids int32 [top_k], dists float32 [top_k]) of sorted keys, padded with -1 / +inf."""
    ids, dists = np.full(top_k, -1, dtype=np.int32), np.full(top_k, np.inf, dtype=F32)
    keys = keys[:top_k]
    ids[:len(keys)] = (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32)
    dists[:len(keys)] = (keys >> np.uint64(32)).astype(np.uint32).view(F32)
    return ids, dists


def search_at(c, qs, probes, ks, id_offset=0):
    """{k: (ids int32 [nq][k], dists float32 [nq][k])} for every k of ks: a row's keys are sorted once."""
    out = {k: (np.empty((len(qs), k), dtype=np.int32), np.empty((len(qs), k), dtype=F32)) for k in ks}
    for i, (q, row) in enumerate(zip(qs, probes)):
        keys = row_keys(c, q, row, id_offset)
        for k in ks:
            out[k][0][i], out[k][1][i] = cut(keys, k)
    return out


def search(c, qs, probes, top_k, id_offset=0):
    """(ids int32 [nq][top_k], dists float32 [nq][top_k]) by key (distance bits, id), padded with -1 / +inf."""
    return search_at(c, qs, probes, (top_k,), id_offset)[top_k]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
