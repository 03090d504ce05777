"""The narrowing and widening rules of the half-precision exact search (include/deltapq_amd.h) restated in numpy (written
from the rules, test infrastructure).

Narrowing is round to nearest, ties to even.  bf16: with u the fp32 bits, (u + 0x7fff + ((u >> 16) & 1)) >> 16.  fp16: the
IEEE conversion -- the value is rounded to a multiple of the half's quantum at its magnitude (2^(e - 10) for 2^e <= |x| <
2^(e + 1) with e >= -14, 2^-24 below: gradual underflow), and a result of 2^16 or more is an infinity.  -0.0 keeps its
sign.  NaNs are out of scope.  Widening is exact: bf16 bits are the upper half of the fp32 bits; an fp16 pattern with
exponent field e and fraction m stands for (1 + m / 1024) * 2^(e - 15), for m / 1024 * 2^-14 when e == 0, and for an
infinity when e == 31.
"""
import numpy as np

FORMATS = ("f16", "bf16")
# the edge values of the contract that stay finite in both formats, and those that narrow to an fp16 infinity
EDGES = np.array([2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 65519.99, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
                  1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 0.0, -0.0, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11),
                  2.0 ** -15, 3 * 2.0 ** -25, 65504.0, -65519.99, -(2.0 ** -24), 1e-30, -1e-30, 2.0 ** -126, 2.0 ** -140],
                 dtype=np.float32)
EDGES_TO_INF = np.array([65520.0, -65520.0, 1e30], dtype=np.float32)   # 1e30 stays finite in bf16


def narrow(a, fmt):
    """float32 array -> uint16 bits of the narrowed values."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    if fmt == "bf16":
        return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    assert fmt == "f16"
    sign = ((u >> np.uint64(16)) & np.uint64(0x8000)).astype(np.uint16)
    x = np.abs(a.astype(np.float64))                       # exact; everything below is exact in fp64 but the one rint
    assert not np.isnan(x).any()
    _, e = np.frexp(x)                                     # x = f * 2^e with 0.5 <= f < 1: 2^(e - 1) <= x
    quantum = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    r = np.rint(x / quantum)                               # round half to even
    val = r * quantum
    out = np.zeros(a.shape, dtype=np.uint16)
    sub = val < 2.0 ** -14
    out[sub] = r[sub].astype(np.uint16)                    # subnormal halves (and zero): the count of 2^-24 quanta
    nor = ~sub & (val < 2.0 ** 16)
    f2, e2 = np.frexp(val[nor])                            # val = (2 f2) * 2^(e2 - 1)
    out[nor] = (((e2 - 1 + 15) << 10) + np.rint((2 * f2 - 1) * 1024).astype(np.int64)).astype(np.uint16)
    out[val >= 2.0 ** 16] = 0x7C00
    return out | sign


def widen(bits, fmt):
    """uint16 bits -> the float32 values they stand for."""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    if fmt == "bf16":
        return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert fmt == "f16"
    e = ((b >> 10) & 31).astype(np.int64)
    m = (b & 0x3FF).astype(np.float64)
    mag = np.where(e == 0, np.ldexp(m / 1024, -14), np.ldexp(1 + m / 1024, e - 15))
    mag = np.where(e == 31, np.inf, mag)                   # NaN patterns (e == 31, m != 0) are out of scope
    return np.where(b & 0x8000, -mag, mag).astype(np.float32)


def not_nan_patterns(fmt):
    """Every 16-bit pattern of the format that is not a NaN."""
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    if fmt == "f16":
        return b[~((((b >> 10) & 31) == 31) & ((b & 0x3FF) != 0))]
    return b[~((((b >> 7) & 255) == 255) & ((b & 0x7F) != 0))]
