"""The rules of the scalar quantiser behind the exact search over 8-bit and 4-bit rows (include/deltapq_amd.h,
"scalar-quantised vectors") restated in numpy (written from the rules, test infrastructure).

bits is 8 or 4 and L = 2^bits - 1.  Train: lo[d] = min, hi[d] = max of the column, -0.0 read as +0.0; step[d] =
(float)(((double)hi - (double)lo) / L).  Encode: code 0 where step == 0, otherwise rint(((double)v - (double)lo) /
(double)step), ties to even, clamped to [0, L].  Decode: lo + (float)c * step in fp32, the product and the sum each rounded
on its own.  Storage: a byte per dimension at 8 bits; at 4 bits dimension 2j in the low and 2j + 1 in the high nibble of
byte j, the spare nibble of an odd D written as 0 and ignored when read.
"""
import numpy as np

BITS = (8, 4)


def levels(bits):
    assert bits in BITS
    return (1 << bits) - 1


def train(rows, bits):
    """float32 [n][D] -> (lo, step), float32 [D] each."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    lo, hi = rows.min(axis=0), rows.max(axis=0)
    lo = np.where(lo == 0, np.float32(0), lo).astype(np.float32)          # -0.0 is stored as +0.0
    hi = np.where(hi == 0, np.float32(0), hi).astype(np.float32)
    step = ((hi.astype(np.float64) - lo.astype(np.float64)) / np.float64(levels(bits))).astype(np.float32)
    return lo, step


def codes(rows, lo, step, bits):
    """float32 [n][D] -> the code of every value, uint8 [n][D], one per byte whatever the width."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    lo, step = np.asarray(lo, dtype=np.float32), np.asarray(step, dtype=np.float32)
    live = step != 0
    safe = np.where(live, step, np.float32(1)).astype(np.float64)
    u = (rows.astype(np.float64) - lo.astype(np.float64)) / safe
    c = np.clip(np.rint(u), 0.0, float(levels(bits)))                     # np.rint: ties to even
    return np.where(live, c, 0.0).astype(np.uint8)


def pack(c, bits):
    """One code per byte [n][D] -> the stored rows: as they are at 8 bits, two to a byte at 4 bits."""
    c = np.ascontiguousarray(c, dtype=np.uint8)
    if bits == 8:
        return c
    n, D = c.shape
    even = np.zeros((n, (D + 1) // 2 * 2), dtype=np.uint8)
    even[:, :D] = c
    return (even[:, 0::2] | (even[:, 1::2] << 4)).astype(np.uint8)


def unpack(stored, D, bits):
    """The stored rows -> one code per byte [n][D]; the spare nibble of an odd D is dropped."""
    stored = np.ascontiguousarray(stored, dtype=np.uint8)
    if bits == 8:
        assert stored.shape[1] == D
        return stored
    assert stored.shape[1] == (D + 1) // 2
    out = np.empty((stored.shape[0], stored.shape[1] * 2), dtype=np.uint8)
    out[:, 0::2] = stored & 15
    out[:, 1::2] = stored >> 4
    return out[:, :D]


def encode(rows, lo, step, bits):
    """float32 [n][D] -> the stored rows, uint8 [n][D] or [n][(D + 1) / 2]."""
    return pack(codes(rows, lo, step, bits), bits)


def decode(stored, lo, step, bits):
    """The stored rows -> float32 [n][D]."""
    lo, step = np.asarray(lo, dtype=np.float32), np.asarray(step, dtype=np.float32)
    c = unpack(stored, lo.shape[0], bits).astype(np.float32)
    prod = (c * step).astype(np.float32)                                  # float32 * float32 -> a rounded float32
    return (lo + prod).astype(np.float32)
