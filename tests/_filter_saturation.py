"""The scan filter's saturations per (slot, sub-space) at M = 8, restated in numpy for tests/test_filter_saturation.py (CPU)
and tests/test_filter_saturation_gpu.py: Cfg<8>'s geometry, filter_scale / filter_offset / row_stat_kernel /
filter_row_stat / filter_saturations of deltapq_amd/csrc/dpq_kernels.hip, the table classes of the tests, and the inverse of
Cfg::slot_of_table that unpacks dpq_debug_filter_tables.  No tests in here.

The rule: stat_m = the 32nd largest of x_m[k] = trunc(clamp(fma(T[m][k], s32, off_m), 0, QT + 1)) over the
row (= x of the row's 32nd largest entry, which row_stat_kernel finds once per batch); SAT_m = SAT_BUDGET stat_m / sum of the stats, capped at QT + 1 with the capped rows' surplus split again; what the
integer divisions drop goes one unit each to the first rows below the cap; no scale or all statistics zero: uniform.
"""
import numpy as np

# ---- Cfg<8> ----------------------------------------------------------------------------------------------------------------
M = 8
QT = 88
XMAX, XU = 7, 1
BIAS = 127 - (QT + 1)
SAT_BUDGET = 255 - BIAS - XMAX * XU
SAT_UNIFORM = SAT_BUDGET // M
SAT_CAP = QT + 1
RANK = 32
QG, NG, AB, F, J = 64, 4, 8, 4, 8            # queries per group, 16-byte entries per (m, code), Cfg::AB / F / J
NO_KEY = 0xFFFFFFFFFFFFFFFF
FLT_MAX = float(np.finfo(np.float32).max)


def uniform():
    return [SAT_UNIFORM] * M


def _bits_step(v, step):
    """float32 v with its bit pattern moved by `step`, as the kernels' __uint_as_float(__float_as_uint(v) + step)."""
    return np.uint32((int(np.float32(v).view(np.uint32)) + step) & 0xFFFFFFFF).view(np.float32)


def filter_scale(mins, key):
    """(s32 float32, bias, B float64) of filter_scale<8>: mins float32 [M], key = the u64 threshold key."""
    B = np.float64(0.0)
    for m in range(M):
        B = B + np.float64(mins[m])
    thr = np.uint32(int(key) >> 32).view(np.float32) if int(key) != NO_KEY else np.float32(0)
    with np.errstate(all="ignore"):
        taup = np.float64(thr) * np.float64(1.0 + 2.0 ** -20)
        R = taup - B
        if int(key) != NO_KEY and R > 0.0 and R < 1e300:
            s = np.float32(np.float64(QT) / R * np.float64(1.0 - 2.0 ** -20))
            if s <= np.float32(FLT_MAX):
                return s, BIAS, B
    return np.float32(0.0), 0, B


def filter_offset(s32, bias, mn, m):
    """filter_offset<8>: the additive term of sub-space m's fma (bias of m = 0 and half a unit folded in, rounded down)."""
    mn = np.float32(mn) if s32 != 0 else np.float32(0.0)
    od = np.float64(mn) * np.float64(s32)
    of = np.float32(od)
    if np.float64(of) < od:
        of = _bits_step(of, 1)
    sd = (np.float64(bias) if m == 0 else np.float64(0.0)) - 0.5 - np.float64(of)
    sf = np.float32(sd)
    if np.float64(sf) > sd:
        sf = _bits_step(sf, -1 if sf > 0 else 1)
    return sf


def fma32(t, s, o):
    """float32 fma(t, s, o), t an array: the product of two fp32 values is exact in the x87 extended format (48 of 64 bits),
    the sum is rounded to 64 bits and then to 24 -- a double rounding only where the 64-bit sum lands on an fp32 midpoint
    that the exact sum missed by less than 2^-40 of it."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended long double"
    with np.errstate(all="ignore"):
        return (np.asarray(t, dtype=np.float32).astype(np.longdouble) * np.longdouble(s) + np.longdouble(o)).astype(np.float32)


def row_stats(T, mins, s32):
    """[M] ints: filter_row_stat of row_stat_kernel's entry of every row (s32 != 0) -- x is monotone in the entry, so the
    32nd largest x of a row is x of its 32nd largest entry."""
    out = []
    for m in range(M):
        entry = np.sort(T[m])[::-1][RANK - 1]
        v = fma32(np.array([entry]), s32, filter_offset(s32, 0, mins[m], 1))[0]
        x = np.float32(SAT_CAP) if np.isnan(v) else min(v, np.float32(SAT_CAP))                  # fminf: NaN -> the cap
        out.append(int(max(x, np.float32(0.0))))                                                  # truncation
    return out


def saturations_of_stats(stat):
    """filter_saturations<8>: eight ints from the eight statistics (integers 0 .. QT + 1)."""
    if not any(stat):
        return uniform()
    sat = [0] * M
    open_ = list(range(M))
    rem = SAT_BUDGET
    while open_:
        S = sum(stat[m] for m in open_)
        if S == 0:
            for m in open_:
                sat[m] = min(rem // len(open_), SAT_CAP)
            break
        capped = [m for m in open_ if rem * stat[m] >= SAT_CAP * S]
        if not capped:
            for m in open_:
                sat[m] = rem * stat[m] // S
            break
        for m in capped:
            sat[m] = SAT_CAP
        rem -= SAT_CAP * len(capped)
        open_ = [m for m in open_ if m not in capped]
    left = SAT_BUDGET - sum(sat)
    for m in range(M):
        if left > 0 and sat[m] < SAT_CAP:
            sat[m] += 1
            left -= 1
    return sat


def saturations(T, key):
    """The eight saturations of a slot: T float32 [M][256] (+inf beyond K), key its u64 threshold key."""
    T = np.asarray(T, dtype=np.float32)
    mins = T.min(axis=1)
    s32, _, _ = filter_scale(mins, key)
    if s32 == 0:
        return uniform()
    return saturations_of_stats(row_stats(T, mins, s32))


def key_of(tau):
    """The threshold key of distance tau with the largest id, as the bootstrap writes it."""
    return (int(np.float32(tau).view(np.uint32)) << 32) | 0xFFFFFFFF


# ---- table classes ---------------------------------------------------------------------------------------------------------
# Entries are multiples of 2^-8 below 2^22 (or +inf): every sum of eight is exact in fp32's 24 bits or rounds once from an
# exact fp64 sum in any order, so the GPU's lists can be held to the oracle's bit for bit.

def _grid(t):
    return (np.rint(np.asarray(t, dtype=np.float64) * 256.0) / 256.0).astype(np.float32)


def _pad(t, K):
    out = np.full(t.shape[:-1] + (256,), np.inf, dtype=np.float32)
    out[..., :K] = t[..., :K]
    return out


def class_tables(name, nq, seed=0):
    """(tables float32 [nq][M][256] with +inf beyond K, K) of one class."""
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    K = 256
    if name == "random":
        t = rng.gamma(2.0, 20.0, size=(nq, M, 256)) * rng.uniform(0.2, 3.0, size=(nq, M, 1))
    elif name == "constant_rows":
        t = np.repeat(rng.integers(1, 500, size=(nq, M, 1)).astype(np.float64), 256, axis=2)
    elif name == "one_wide_row":
        t = np.repeat(rng.integers(1, 50, size=(nq, M, 1)).astype(np.float64), 256, axis=2)
        wide = rng.integers(0, M, size=nq)
        t[np.arange(nq), wide] = rng.uniform(0.0, 4000.0, size=(nq, 256))
    elif name == "two_valued":
        t = np.where(rng.random((nq, M, 256)) < 0.5, 0.0, 2.0 ** 21)
        t[:, :, 0] = 0.0
    elif name in ("inf_beyond_16", "inf_beyond_200"):
        K = 16 if name == "inf_beyond_16" else 200
        t = rng.gamma(2.0, 20.0, size=(nq, M, 256))
    elif name == "clustered":
        # bench-shaped: squared distances of a query to the 256 centroids of a clustered sub-space
        cen = rng.normal(0.0, 4.0, size=(M, 256, 16)) + rng.normal(0.0, 12.0, size=(M, 8, 16))[:, rng.integers(0, 8, 256)]
        q = cen[np.arange(M)[None, :], rng.integers(0, 256, size=(nq, M))] + rng.normal(0.0, 3.0, size=(nq, M, 16))
        t = ((cen[None] - q[:, :, None, :]) ** 2).sum(axis=3)
    else:
        raise KeyError(name)
    return _pad(_grid(t), K), K


CLASSES = ("random", "constant_rows", "one_wide_row", "two_valued", "inf_beyond_16", "inf_beyond_200", "clustered")


# ---- dpq_debug_filter_tables ------------------------------------------------------------------------------------------------

def slot_of_table(g, c, tb):
    """Cfg<8>::slot_of_table: byte tb of dword c of 16-byte entry g -> local slot (R = 1: accumulator 4 g + c, field tb)."""
    acc, f = 4 * g + c, tb
    return (acc // AB) * (J * F) + f * J + acc % AB


def unpack_tables(raw, n_groups):
    """(entries uint8 [slots][M][256], sat uint8 [slots][M], keys uint64 [slots]) from the hook's bytes: tables
    [group][g][m][code] x 16 B in the LDS layout, then one (8 saturation bytes, u64 key) record per slot."""
    raw = np.frombuffer(raw, dtype=np.uint8)
    nt = n_groups * NG * M * 256 * 16
    tab = raw[:nt].reshape(n_groups, NG, M, 256, 4, 4)                    # [group][g][m][code][c][tb]
    entries = np.empty((n_groups * QG, M, 256), dtype=np.uint8)
    for g in range(NG):
        for c in range(4):
            for tb in range(4):
                ls = slot_of_table(g, c, tb)
                entries[ls::QG] = tab[:, g, :, :, c, tb]
    rec = raw[nt:nt + n_groups * QG * 16].reshape(n_groups * QG, 16)
    return entries, rec[:, :8].copy(), rec[:, 8:].copy().view(np.uint64).reshape(-1)
