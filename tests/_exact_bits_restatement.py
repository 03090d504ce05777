"""The binary-vector rules of include/deltapq_amd.h ("binary vectors") restated in numpy (written from the rules, test
infrastructure).

A row is D bits in (D + 7) // 8 bytes, dimension d in bit d & 7 of byte d >> 3; the spare bits of the last byte are
ignored.  The distance of a query and a row is the number of differing dimensions, an integer, reported as float32.  A
result list is the k smallest keys `distance bits << 32 | id` in ascending order: (distance, id), the lowest ids first
among equal distances; short lists are padded with -1 / +inf.  Range search keeps d < r, strictly.  Re-ranking follows
_exact_restatement.rerank: the map, the even-N rule, padding candidates, a row named twice counting once.
"""
import numpy as np


def n_bytes(D):
    return (D + 7) // 8


def mask_spare(packed, D):
    """The packed rows with the spare bits of the last byte cleared."""
    p = np.array(packed, dtype=np.uint8, copy=True)
    assert p.ndim == 2 and p.shape[1] == n_bytes(D)
    if D % 8:
        p[:, -1] &= np.uint8((1 << (D % 8)) - 1)
    return p


def unpack_bits(packed, D):
    """uint8 0/1 [n][D]."""
    return np.unpackbits(mask_spare(packed, D), axis=1, bitorder="little")[:, :D]


def pack_bits(bits01):
    """0/1 [n][D] -> packed uint8 [n][(D + 7) // 8], spare bits 0."""
    return np.packbits(np.asarray(bits01, dtype=np.uint8), axis=1, bitorder="little")


def all_distances(base, queries, D):
    """float32 [nq][n]: XOR and sum in int64, then the float distance."""
    b, q = unpack_bits(base, D), unpack_bits(queries, D)
    out = np.empty((len(q), len(b)), dtype=np.int64)
    for i, row in enumerate(q):
        out[i] = (b ^ row[None, :]).sum(axis=1, dtype=np.int64)
    return out.astype(np.float32)


def _ordered(d, ids):
    """(distance, id) ascending, by a stable sort of the ids under a stable sort of the distances."""
    by_id = np.argsort(ids, kind="stable")
    order = by_id[np.argsort(d[by_id], kind="stable")]
    return d[order], ids[order]


def _pad(d, ids, top_k):
    out_i = np.full(top_k, -1, dtype=np.int32)
    out_d = np.full(top_k, np.inf, dtype=np.float32)
    m = min(top_k, len(ids))
    out_i[:m] = ids[:m]
    out_d[:m] = d[:m]
    return out_i, out_d


def search(base, queries, D, top_k, id_offset=0, allowed=None, dist=None):
    """ids int32 [nq][top_k], dists float32 [nq][top_k].  allowed: bool [n] over rows, or None for all of them."""
    dist = all_distances(base, queries, D) if dist is None else dist
    rows = np.arange(dist.shape[1], dtype=np.int64)
    if allowed is not None:
        rows = rows[np.asarray(allowed, dtype=bool)]
    out_i, out_d = [], []
    for dq in dist:
        d, ids = _ordered(dq[rows], rows + id_offset)
        i, dd = _pad(d, ids, top_k)
        out_i.append(i)
        out_d.append(dd)
    return np.stack(out_i), np.stack(out_d)


def allowed_rows(n, id_offset, mask):
    """bool [n]: row r is allowed when mask[r + id_offset] is set; ids at or beyond len(mask) are not."""
    mask = np.asarray(mask, dtype=bool)
    ids = np.arange(n, dtype=np.int64) + id_offset
    ok = ids < len(mask)
    out = np.zeros(n, dtype=bool)
    out[ok] = mask[ids[ok]]
    return out


def range_search(base, queries, D, radii, id_offset=0, allowed=None, dist=None):
    """(lims int64 [nq + 1], ids int32, dists float32): every (allowed) row with d < radius, by (distance, id)."""
    dist = all_distances(base, queries, D) if dist is None else dist
    nq = dist.shape[0]
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (nq,))
    rows = np.arange(dist.shape[1], dtype=np.int64)
    if allowed is not None:
        rows = rows[np.asarray(allowed, dtype=bool)]
    lims, ids, ds = [0], [], []
    for dq, r in zip(dist, radii):
        keep = dq[rows] < r
        d, i = _ordered(dq[rows][keep], rows[keep] + id_offset)
        ids.append(i.astype(np.int32))
        ds.append(d.astype(np.float32))
        lims.append(lims[-1] + len(i))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(ids) if ids else np.zeros(0, np.int32),
            np.concatenate(ds) if ds else np.zeros(0, np.float32))


def rerank(base, queries, D, cand, top_k, id_offset=0, id_map=None):
    """dpq_flat_rerank's rules (see _exact_restatement.rerank) under the Hamming distance."""
    b = unpack_bits(base, D)
    out_i, out_d = [], []
    for q, cs in zip(unpack_bits(queries, D), np.asarray(cand)):
        cs = cs[cs >= 0].astype(np.int64)
        if id_map is not None:
            n_map = len(id_map)
            if n_map % 2 == 0:
                cs = np.where(cs == n_map, n_map - 1, cs)
            rows = np.asarray(id_map, dtype=np.int64)[cs]
        else:
            rows = cs - id_offset
        rows = np.unique(rows)
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < len(b))
        d = (b[rows] ^ q[None, :]).sum(axis=1, dtype=np.int64).astype(np.float32)
        dd, ids = _ordered(d, rows + id_offset)
        i, dd = _pad(dd, ids, top_k)
        out_i.append(i)
        out_d.append(dd)
    return np.stack(out_i), np.stack(out_d)


def from_float(vectors, thresholds=None):
    """bit d = v[d] > t[d] in fp32 (t = 0 without thresholds): NaN and -0.0 > 0 give 0.  Packed, spare bits 0."""
    v = np.asarray(vectors, dtype=np.float32)
    t = np.zeros(v.shape[1], dtype=np.float32) if thresholds is None else np.asarray(thresholds, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return pack_bits(v > t[None, :])
