"""The residual re-ranking rules of include/deltapq_amd.h restated in numpy (written from the rules, test infrastructure).

A handle has codewords1 [M][K][Ds] and a level-1 code c1[M] per node; D1 = M * Ds.  A level has codewords2 [M2][K2][Ds2],
Ds2 = ceil(D1 / M2), and a code c2[M2] per node.  For j = 0 .. D1-1:
    a[j] = codewords1[j / Ds][c1[j / Ds]][j % Ds]
    r[j] = v[j] - a[j]           one fp32 subtraction; v zero padded from D to D1
    c2   = the PQ encoder's answer for r over codewords2 (r zero padded from D1 to M2 * Ds2, the first minimum wins)
    b[j] = codewords2[j / Ds2][c2[j / Ds2]][j % Ds2]
    x[j] = a[j] + b[j]           one fp32 add
The refined distance of q to the node is the exact search's arithmetic over the row x (_exact_restatement.distances).
A result list holds the k smallest keys `distance bits << 32 | candidate id`, a node named twice counting once."""
import os
import sys

import numpy as np

import _exact_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pq_encode_oracle as E  # noqa: E402

NAN_BITS = 0x7FC00000


def shape_ok(D1, M2, K2, Ds2):
    """The contract's rules for a level's shape."""
    return 1 <= M2 <= 64 and 2 <= K2 <= 256 and Ds2 == -(-D1 // M2) and (M2 - 1) * Ds2 < D1


def gather(cb, codes, width):
    """float32 [n][width]: the codewords the codes name, side by side, cut to `width` columns."""
    cb = np.asarray(cb, dtype=np.float32)
    rows = np.concatenate([cb[m, codes[:, m]] for m in range(cb.shape[0])], axis=1)
    return np.ascontiguousarray(rows[:, :width])


def level1(cb1, codes1):
    """a rows [n][D1]."""
    return gather(cb1, codes1, cb1.shape[0] * cb1.shape[2])


def residuals(vectors, cb1, codes1):
    """r rows [n][D1] of vectors [n][D] against the nodes' level-1 codes."""
    a = level1(cb1, codes1)
    v = np.zeros_like(a)
    vv = np.asarray(vectors, dtype=np.float32)
    assert -(-vv.shape[1] // cb1.shape[0]) == cb1.shape[2], "ceil(D / M) must be Ds"
    v[:, :vv.shape[1]] = vv
    return (v - a).astype(np.float32)


def encode2(res, cb2):
    """c2 uint8 [n][M2]: the encoder over the residual rows (it pads them to M2 * Ds2 itself)."""
    return E.encode_pq(res, cb2)


def reconstruct(cb1, codes1, cb2, codes2):
    """x rows [n][D1]."""
    a = level1(cb1, codes1)
    b = gather(cb2, codes2, a.shape[1])
    return (a + b).astype(np.float32)


def local_of(ids, node_lo, node_hi, n_total, even_rule=True):
    """int64 local positions of reported ids, -1 where an id names no node of the handle [node_lo, node_hi) of an
    index of n_total codes (even rule: id N names position N - 1 and N - 1 nothing)."""
    pos = np.asarray(ids, dtype=np.int64).copy()
    if even_rule and n_total % 2 == 0:
        hole = pos == n_total - 1
        pos[pos == n_total] = n_total - 1
        pos[hole] = -1
    ok = (pos >= node_lo) & (pos < node_hi)
    return np.where(ok, pos - node_lo, -1)


def rerank(xrows, queries, cand, top_k, node_lo=0, n_total=None, even_rule=True):
    """ids int32 [nq][top_k], dists fp32 [nq][top_k] over xrows (the handle's x rows by local position).  Negative
    candidates are padding; the reported id is the candidate's; a node named twice counts once."""
    n_total = len(xrows) + node_lo if n_total is None else n_total
    out_i, out_d = [], []
    for q, cs in zip(np.asarray(queries, dtype=np.float32), np.asarray(cand)):
        cs = np.unique(cs[cs >= 0].astype(np.int64))
        loc = local_of(cs, node_lo, node_lo + len(xrows), n_total, even_rule)
        assert (loc >= 0).all(), "a candidate names no node"
        d = X.distances(xrows[loc], q) if len(cs) else np.zeros(0, dtype=np.float32)
        i, dd = X.unpack(np.sort(X.keys(d, cs)), top_k)
        out_i.append(i)
        out_d.append(dd)
    return np.stack(out_i), np.stack(out_d)


def sample_positions(n_local, train_n):
    """l_i = floor(i * n_local / train_n)."""
    return [(i * n_local) // train_n for i in range(train_n)]
