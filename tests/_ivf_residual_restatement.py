"""The rules of the IVF search by residual (include/deltapq_amd.h "IVF search by residual"), restated in numpy for
tests/test_ivf_residual*.py.  No tests in here, and nothing but numpy.

A case is a dict with cb [M][K][Ds], cents [nlist][M * Ds], offsets and ids (the lists, reported ids), entry_codes (the
code of every list entry, in list order) and plain (the handle's accumulate rule).  r = q - c_l in fp32, the table by the
table build's rule, then the fp64 sum rounded once (a DTC handle) or M fp32 additions (a plain handle); the answer is the
sorted keys (distance bits << 32 | id) of the union of the probed lists, cut at top_k and padded with -1 / +inf.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def table(cb, r):
    """float32 [M][256]: the exact table of the (residual) query r under codebook cb [M][K][Ds]; k >= K: +inf."""
    M, K, Ds = cb.shape
    acc = np.zeros((M, K), dtype=F32)
    for d in range(Ds):
        diff = (cb[:, :, d] - r.reshape(M, Ds)[:, d, None]).astype(F32)            # fp32 subtract
        acc = (acc.astype(F64) + diff.astype(F64) * diff.astype(F64)).astype(F32)  # the square in fp64; float += double
    T = np.full((M, 256), np.inf, dtype=F32)
    T[:, :K] = acc
    return T


def distances(T, codes, plain):
    """float32 [n]: codes uint8 [n][M] under table T, m ascending."""
    e = T[np.arange(T.shape[0]), codes]
    acc = np.zeros(len(codes), dtype=F32 if plain else F64)
    for m in range(T.shape[0]):
        acc = (acc + e[:, m]).astype(acc.dtype)                                    # (f64 + f32 is an f64 addition)
    return acc.astype(F32)


def list_keys(c, q, l):
    """uint64 [len of list l], in list order: the key of every entry of list l for query q."""
    ent = slice(c["offsets"][l], c["offsets"][l + 1])
    d = distances(table(c["cb"], (q - c["cents"][l]).astype(F32)), c["entry_codes"][ent], c["plain"])
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | c["ids"][ent].astype(np.int64).astype(np.uint64)


def row_keys(c, q, row, allowed=None, memo=None, qn=None):
    """uint64 [m], ascending: the keys of the union of the lists the probe row names -- padding (-1) skipped, a repeat
    counted once -- and of the ids `allowed` (bool by id) lets through.  memo (a dict) keeps list_keys by (qn, list): a
    call whose queries cycle through a few distinct ones (qn: which one q is) makes each table once."""
    keys = [np.zeros(0, dtype=np.uint64)]
    for l in dict.fromkeys(int(p) for p in row if p >= 0):
        if memo is None:
            k = list_keys(c, q, l)
        else:
            if (qn, l) not in memo:
                memo[qn, l] = list_keys(c, q, l)
            k = memo[qn, l]
        if allowed is not None:
            k = k[allowed[(k & np.uint64(0xffffffff)).astype(np.int64)]]
        keys.append(k)
    return np.sort(np.concatenate(keys))


def cut(keys, top_k):
    """(ids int32 [top_k], dists float32 [top_k]) of sorted keys, padded with -1 / +inf."""
    ids, dists = np.full(top_k, -1, dtype=np.int32), np.full(top_k, np.inf, dtype=F32)
    keys = keys[:top_k]
    ids[:len(keys)] = (keys & np.uint64(0xffffffff)).astype(np.int32)
    dists[:len(keys)] = (keys >> np.uint64(32)).astype(np.uint32).view(F32)
    return ids, dists


def search_at(c, qs, probes, ks, allowed=None, use=None, memo=None):
    """{k: (ids int32 [nq][k], dists float32 [nq][k])} for every k of ks: a row's keys are sorted once.  use (int [nq]):
    query i is qs[use[i]], and tables are kept in memo (row_keys) by (use[i], list); else query i is qs[i]."""
    nq = len(probes)
    if use is not None and memo is None:
        memo = {}
    out = {k: (np.empty((nq, k), dtype=np.int32), np.empty((nq, k), dtype=F32)) for k in ks}
    for i, row in enumerate(probes):
        qn = i if use is None else int(use[i])
        keys = row_keys(c, qs[qn], row, allowed, memo, qn)
        for k in ks:
            out[k][0][i], out[k][1][i] = cut(keys, k)
    return out


def search(c, qs, probes, top_k, allowed=None):
    """(ids int32 [nq][top_k], dists float32 [nq][top_k]) by key (distance bits, id), padded with -1 / +inf."""
    return search_at(c, qs, probes, (top_k,), allowed)[top_k]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
