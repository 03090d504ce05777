"""What a filter of a handle must hold, restated in plain numpy (tests/test_filter_build.py).  No tests in here.

A handle holds local nodes 0 .. n_local - 1 at global positions base + l.  It reports node l as base + l, except that a
DTC handle (not plain) with even N reports the node at position N - 1 as N."""
import numpy as np


def reported(base, n_local, N, plain):
    r = int(base) + np.arange(n_local, dtype=np.int64)
    if not plain and N % 2 == 0:
        r[r == N - 1] = N
    return r


def local_bits(base, n_local, N, plain, pred):
    """bool [n_local]: pred (int64 array of reported ids -> bool array) of every node's reported id."""
    return np.asarray(pred(reported(base, n_local, N, plain)), dtype=bool).reshape(n_local)


def local_bits_vec(vec_id, pred):
    """The same through a map: pred of every node's original vector id."""
    return np.asarray(pred(np.asarray(vec_id, dtype=np.int64)), dtype=bool).reshape(len(vec_id))


def in_mask(mask):
    """The predicate of a bool array over ids: id < len(mask) and mask[id]."""
    mask = np.asarray(mask, dtype=bool)
    return lambda r: (r < len(mask)) & np.append(mask, False)[np.minimum(r, len(mask))]


def as_reported_mask(bits, base, n_local, N, plain, n_bits):
    """Local bits -> bool [n_bits] over reported ids (what dpq_filter_to_bitmap returns)."""
    r = reported(base, n_local, N, plain)
    out = np.zeros(n_bits, dtype=bool)
    ok = r < n_bits
    out[r[ok]] = np.asarray(bits, dtype=bool)[ok]
    return out
