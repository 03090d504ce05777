"""The rules of the search by distance tables and of the inner-product search (include/deltapq_amd.h "search by distance
tables, and inner product"), restated in numpy for tests/test_tables_search.py and tests/test_ip_search.py.  No tests in
here, and nothing but numpy.

Every function follows its rule operation by operation; numpy's float32 and float64 arithmetic is IEEE round-to-nearest,
so each line below is one rounding of the rule.
"""
import numpy as np

f32, f64 = np.float32, np.float64


def _cb_q(cb, queries):
    cb = np.ascontiguousarray(cb, dtype=f32)
    M, K, Ds = cb.shape
    q = np.ascontiguousarray(queries, dtype=f32)
    if q.ndim == 1:
        q = q[None, :]
    return cb, q.reshape(q.shape[0], M, Ds)


def l2_tables(cb, queries):
    """float32 [nq][M][K]: the L2 table rule of every search (h:2845-2846), T[m][k] from acc32 = +0 by
    acc32 = float32(float64(acc32) + float64(diff32)^2), diff32 = c[m][k][d] - q[m * Ds + d] in fp32, d ascending."""
    cb, q = _cb_q(cb, queries)
    acc = np.zeros((q.shape[0],) + cb.shape[:2], dtype=f32)
    with np.errstate(over="ignore"):
        for d in range(cb.shape[2]):
            diff = cb[None, :, :, d] - q[:, :, None, d]                  # fp32 - fp32: one rounding to fp32
            assert diff.dtype == f32
            sq = diff.astype(f64) * diff.astype(f64)                     # exact: 48 significant bits
            acc = (acc.astype(f64) + sq).astype(f32)                     # float += double
    return acc


def ip_products(cb, queries):
    """float32 [nq][M][K]: p[m][k] = (float)acc, acc = +0.0 in fp64, acc += (double)q[m * Ds + d] * (double)c[m][k][d] for d
    ascending (the product is exact in fp64: one rounding per step)."""
    cb, q = _cb_q(cb, queries)
    acc = np.zeros((q.shape[0],) + cb.shape[:2], dtype=f64)
    for d in range(cb.shape[2]):
        acc = acc + q[:, :, None, d].astype(f64) * cb[None, :, :, d].astype(f64)
    with np.errstate(over="ignore"):
        return acc.astype(f32)


def ip_tables(cb, queries):
    """(p, top float32 [nq][M], e float32 [nq][M][K], B float32 [nq]): top[m] the largest p[m][k], e = top - p in fp32,
    B = (float) of the fp64 sum from +0.0, m ascending, of (double)top[m]."""
    p = ip_products(cb, queries)
    top = p.max(axis=2)
    e = top[:, :, None] - p
    assert e.dtype == f32
    acc = np.zeros(p.shape[0], dtype=f64)
    for m in range(p.shape[1]):
        acc = acc + top[:, m].astype(f64)
    return p, top, e, acc.astype(f32)


def ip_scores(B, gaps, ids):
    """float32 [nq][k] from B [nq], gaps and ids [nq][k]: s = (float)((double)B - (double)g); -inf where the row is padding
    (id < 0)."""
    gaps = np.asarray(gaps, dtype=f32)
    B = np.asarray(B, dtype=f32).reshape(-1, 1)
    s = (B.astype(f64) - gaps.astype(f64)).astype(f32)
    s[np.asarray(ids) < 0] = -np.inf
    return s


def entries(table, codes):
    """float32 [n][M]: table[m][codes[i][m]]."""
    table = np.asarray(table, dtype=f32)
    codes = np.asarray(codes)
    return table[np.arange(codes.shape[1])[None, :], codes]


def distances_dtc(table, codes):
    """float32 [n]: the rule of a DTC handle -- the fp64 sum of the M fp32 entries (m ascending here; for an exact table
    no order rounds), rounded once to fp32."""
    ent = entries(table, codes).astype(f64)
    acc = np.zeros(len(ent), dtype=f64)
    with np.errstate(over="ignore"):
        for m in range(ent.shape[1]):
            acc = acc + ent[:, m]
        return acc.astype(f32)


def distances_plain(table, codes):
    """float32 [n]: the rule of a dpq_open_plain_* handle -- `float dist += lut[m][code]`, m ascending: M fp32 roundings."""
    ent = entries(table, codes)
    acc = np.zeros(len(ent), dtype=f32)
    with np.errstate(over="ignore"):
        for m in range(ent.shape[1]):
            acc = acc + ent[:, m]
            assert acc.dtype == f32
    return acc
