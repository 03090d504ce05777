"""The byte exact-search rules of include/deltapq_amd.h restated in numpy (test infrastructure): the distance is the
integer sum of squared differences converted to fp32, round to nearest even; keys, order, padding and the candidate
rules are _exact_restatement's."""
import numpy as np

import _exact_restatement as X


def distances(base, q):
    """fp32 [n]: base uint8 [n][D], q uint8 [D]."""
    assert base.dtype == np.uint8 and q.dtype == np.uint8
    return ((base.astype(np.int64) - q.astype(np.int64)) ** 2).sum(-1).astype(np.float32)


def search(base, queries, top_k, id_offset=0):
    out_i, out_d = [], []
    rows = np.arange(len(base), dtype=np.int64) + id_offset
    for q in queries:
        i, d = X.unpack(np.sort(X.keys(distances(base, q), rows)), top_k)
        out_i.append(i)
        out_d.append(d)
    return np.stack(out_i), np.stack(out_d)


def rerank(base, queries, cand, top_k, id_offset=0, id_map=None):
    """X.rerank's candidate rules over the widened bytes; every distance it reports is then held to the integer one."""
    assert base.dtype == np.uint8 and queries.dtype == np.uint8
    ids, d = X.rerank(base.astype(np.float32), queries.astype(np.float32), cand, top_k, id_offset=id_offset, id_map=id_map)
    for q, i, dd in zip(queries, ids, d):
        ok = i >= 0
        assert np.array_equal(dd[ok].view(np.uint32), distances(base[i[ok] - id_offset], q).view(np.uint32))
    return ids, d
