"""Distance tables at the numeric edges, for tests/test_numeric_edges.py and scripts/fuzz_parity.py --tables: classes of
codebooks whose tables are exact by construction, the scan paths they are run through, and a reference in exact rational
arithmetic.  No tests in here.

Tables.  A Ds = 1 codebook c[m][k] = j * 2^e with integer |j| < 4096 gives, against the all-zero query, the table
T[m][k] = j^2 * 4^e with no rounding anywhere in the mixed LUT rule (h:2845-2846; the idea of codebook_for_table in
tests/test_hand_derived.py, here for M in {8, 16} and K <= 256).  For any other query the table is worked out by the book
-- fp32 subtract, exact fp64 square, (float)((double)acc + sq) -- on fractions.Fraction with rne(), a round-to-nearest-even
that knows a format's exponent limits: denormals are multiples of 2^-149, what rounds to 2^128 or beyond is +inf.

Reference.  The distance of a code is the exact rational sum of its M table entries rounded ONCE to fp32 (the DTC rule), or
M sequential fp32 roundings in ascending m (the plain index, h:2658-2662).  The answer is the first k of (fp32 bits,
reported id) ascending -- the canonical order of DESIGN.md section 3 -- so expected ids and bits are unique and compared
strictly.  table_units() holds every table to the condition that makes this the reference's own answer too: all entries are
integer multiples of one power of two and every sum of M of them stays below 2^53 units, so the oracle's incremental fp64
stack never rounds (tests/test_numeric_edges.py demands the oracle's bits equal these, no tolerance, no exempt rows).
+inf entries are ordinary values; the trees of the `overflow` class never replace one (inf - inf would be the reference's
NaN, which is out of scope: include/deltapq_amd.h "Result semantics").

Choices the issue leaves open, and why:
 * `ulp_crowd` puts T[0][.] = 9 * 2^20 = (3 * 2^10)^2 where the issue writes 2^23: 2^23 is not the square of a float, and
   9 * 2^20 lies in the same binade [2^23, 2^24), where consecutive fp32 values are consecutive integers.
 * `fp32_ties` has T[0][k] = j^2 * 2^30 with j in {1, 2, 3} (squares again).
 * the ladders draw their exponent level as floor(25 u^(M/4)), u uniform: most codewords sit low, so that the best codes of
   a few thousand reach the bottom of the ladder (at a uniform draw the top-10 of 4097 codes would start 12 levels up), and
   the chance that all M entries of a code lie below a level is the same at M = 8 and M = 16.
 * queries of every class, in this order: the all-zero query, the sub-vectors of one code of the index (a distance-0 hit),
   a far query, the sub-vectors of a second code.  A batch of nq queries cycles through them.
 * the Python restatement of the oracle decodes M = 8 streams only, and slowly: it is checked on the first SMALL_N codes.
"""
import math
from fractions import Fraction as F

import numpy as np

INF = math.inf          # +inf among the exact rationals
SMALL_N = 301
N_SCAN, N_BOOT = 4097, 17001      # the smallest sizes at which the paths below exist (17 001: a bootstrap = 1 shard needs 16 K nodes)


# ---- exact arithmetic ----------------------------------------------------------------------------------------------------

def rne(x, p, emin, emax):
    """The rational x rounded to the nearest number of a binary format with a p-bit significand, ties to even: normal
    numbers 2^emin .. below 2^(emax + 1), denormals as multiples of 2^(emin - p + 1), and +-INF for what rounds to
    2^(emax + 1) or beyond (IEEE 754 round-to-nearest).  INF stays INF."""
    if x == INF or x == -INF:
        return x
    x = F(x)
    if x == 0:
        return F(0)
    s = 1 if x > 0 else -1
    num, den = abs(x.numerator), x.denominator
    e = num.bit_length() - den.bit_length()            # 2^(e-1) < x < 2^(e+1)
    if (num < den << e) if e >= 0 else (num << -e < den):
        e -= 1                                         # 2^e <= x < 2^(e+1)
    qe = max(e, emin) - p + 1                          # the quantum is 2^qe
    if qe >= 0:
        den <<= qe
    else:
        num <<= -qe
    n, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and n & 1):
        n += 1
    if n.bit_length() + qe > emax + 1:                 # n * 2^qe >= 2^(emax + 1)
        return s * INF
    return s * (F(n) * F(2) ** qe)


def rne32(x):
    return rne(x, 24, -126, 127)


def rne64(x):
    return rne(x, 53, -1022, 1023)


def to_f32(x):
    """numpy.float32 of a rational that IS an fp32 value (asserted), or of +-INF."""
    if x == INF or x == -INF:
        return np.float32(x)
    assert rne32(x) == x
    return np.float32(x.numerator / x.denominator)     # int / int is correctly rounded to double, which holds every fp32 value


def from_f32(v):
    v = float(v)
    return v if math.isinf(v) else F(v)


def table_by_the_book(cb, q):
    """[M][K] rationals (or INF): h:2845-2846 `m_sub_distances[i][j] += pow(m_codewords[i][j][k] - query[i*m_Ds+k], 2)` with
    a float accumulator -- float - float (one rounding to fp32), pow(double, 2) (the square of a 24-bit value is exact in
    double), float += double = (double)acc + sq rounded to double, then stored as float."""
    cb = np.asarray(cb, dtype=np.float32)
    M, K, Ds = cb.shape
    q = np.asarray(q, dtype=np.float32).reshape(M, Ds)
    T = []
    for m in range(M):
        qm = [from_f32(v) for v in q[m]]
        row = []
        for k in range(K):
            acc = F(0)
            for d in range(Ds):
                diff = rne32(from_f32(cb[m, k, d]) - qm[d])
                sq = diff * diff
                assert rne64(sq) == sq
                acc = rne32(rne64(acc + sq))
            row.append(acc)
        T.append(row)
    return T


def table_by_construction(J, E):
    """[M][K] rationals j^2 * 4^e: the table of grid_codebook(J, E) against the all-zero query."""
    J, E = np.asarray(J), np.broadcast_to(np.asarray(E), np.shape(J))
    return [[F(int(j) * int(j)) * F(4) ** int(e) for j, e in zip(jr, er)] for jr, er in zip(J, E)]


def grid_codebook(J, E):
    """float32 [M][K][1]: c = j * 2^e, |j| < 4096 (asserted: j^2 then has at most 24 bits)."""
    J = np.asarray(J, dtype=np.int64)
    assert np.all(np.abs(J) < 4096)
    cb = np.ldexp(J.astype(np.float64), np.broadcast_to(np.asarray(E, dtype=np.int64), J.shape)).astype(np.float32)
    assert np.all(np.isfinite(cb)) and np.all((cb != 0) == (J != 0))
    return cb[:, :, None]


def np_table(T):
    return np.array([[to_f32(v) for v in row] for row in T], dtype=np.float32)


def table_units(T):
    """(units int64 [M][K], is_inf bool [M][K], g): every finite entry is units * 2^g exactly.  Asserts the condition under
    which fp64 sums of the entries are exact in any order: M maxima together stay below 2^53 units."""
    g = None
    for row in T:
        for v in row:
            if v != INF and v != 0:
                tz = (v.numerator & -v.numerator).bit_length() - 1
                low = tz - (v.denominator.bit_length() - 1)
                assert v.denominator & (v.denominator - 1) == 0
                g = low if g is None else min(g, low)
    g = 0 if g is None else g
    M, K = len(T), len(T[0])
    units = np.zeros((M, K), dtype=np.int64)
    is_inf = np.zeros((M, K), dtype=bool)
    total = 0
    for m in range(M):
        top = 0
        for k in range(K):
            if T[m][k] == INF:
                is_inf[m, k] = True
                continue
            u = T[m][k] / F(2) ** g
            assert u.denominator == 1
            top = max(top, int(u))
            units[m, k] = int(u) if int(u) < 2 ** 62 else -1
        total += top
    assert total < 2 ** 53, "the table's span is too wide for exact fp64 sums: %d units" % total
    return units, is_inf, g


def _round_units(s, g):
    """float32 array: the int64 sums s (in units of 2^g) rounded to fp32 with rne32, one call per distinct sum."""
    uniq, inv = np.unique(s, return_inverse=True)
    vals = np.array([to_f32(rne32(F(int(u)) * F(2) ** g)) for u in uniq], dtype=np.float32)
    return vals[inv.reshape(-1)]


def exact_distances(T, codes):
    """float32 [n]: the DTC rule -- the exact sum of the M entries, rounded once."""
    units, is_inf, g = table_units(T)
    codes = np.asarray(codes)
    mm = np.arange(codes.shape[1])
    d = _round_units(units[mm, codes].sum(axis=1), g)
    d[is_inf[mm, codes].any(axis=1)] = np.inf
    return d


def exact_distances_fp32_rule(T, codes):
    """float32 [n]: the plain index (h:2658-2662) -- `float dist += lut[m][code]`, m ascending: M roundings to fp32.  Every
    partial sum is an fp32 value above the unit 2^g, so it is again a whole number of units."""
    units, is_inf, g = table_units(T)
    codes = np.asarray(codes)
    n, M = codes.shape
    acc = np.zeros(n, dtype=np.int64)
    dead = np.zeros(n, dtype=bool)                    # +inf so far
    scale = F(2) ** g
    for m in range(M):
        dead |= is_inf[m, codes[:, m]]
        s = acc + units[m, codes[:, m]]
        uniq, inv = np.unique(s, return_inverse=True)
        nxt = np.zeros(len(uniq), dtype=np.int64)
        over = np.zeros(len(uniq), dtype=bool)
        for i, u in enumerate(uniq):
            r = rne32(F(int(u)) * scale)
            if r == INF:
                over[i] = True
            else:
                r = r / scale
                assert r.denominator == 1
                nxt[i] = int(r)
        inv = inv.reshape(-1)
        acc = nxt[inv]
        dead |= over[inv]
    d = _round_units(acc, g)                           # (already fp32 values: this rounding changes nothing)
    d[dead] = np.inf
    return d


# ---- trees ---------------------------------------------------------------------------------------------------------------

def tree_parts(tree):
    """(bits bool [n][M], vals uint8 [n][M]): which positions every node changes, and to what."""
    M, masks = tree["M"], tree["masks"]
    bits = ((masks[:, None] >> np.arange(M)[None, :]) & 1).astype(bool)
    bits[0] = False
    vals = np.zeros(bits.shape, dtype=np.uint8)
    vals[bits] = tree["deltas"]
    return bits, vals


def tree_from_parts(root, depths, bits, vals, M):
    bits = bits.copy()
    bits[0] = False
    masks = (bits * (1 << np.arange(M)).astype(np.uint32)).sum(axis=1).astype(np.uint16)
    return dict(root=np.asarray(root, dtype=np.uint8), depths=np.asarray(depths, dtype=np.uint8), masks=masks,
                deltas=np.ascontiguousarray(vals[bits], dtype=np.uint8), M=M)


def plain_tree(n, M, K, seed, mean_diffs=3.0):
    """synth.synth_tree with its bytes reduced mod K."""
    from deltapq_amd import synth
    tree = synth.synth_tree(n, M, seed=seed, mean_diffs=mean_diffs)
    tree["deltas"] = (tree["deltas"].astype(np.int64) % K).astype(np.uint8)
    tree["root"] = (tree["root"].astype(np.int64) % K).astype(np.uint8)
    return tree


def tree_with_copies_of_the_root(n, M, K, seed, copies):
    """A duplicate-heavy tree in which `copies` nodes, spread over the index, are depth-1 children of the root that change
    nothing (fewer where the index is too short to hold them)."""
    tree = plain_tree(n, M, K, seed, mean_diffs=0.35)
    bits, vals = tree_parts(tree)
    depths = tree["depths"].copy()
    nxt = np.append(depths[2:], 1)[:n - 1]                                         # depth of the node after node i, i >= 1
    ok = 1 + np.flatnonzero(nxt <= 2)                                               # ... which must stay <= depth(i) + 1
    if len(ok):
        pick = ok[np.unique(np.linspace(0, len(ok) - 1, min(copies, len(ok))).astype(np.int64))]
        depths[pick] = 1
        bits[pick] = False
    return tree_from_parts(tree["root"], depths, bits, vals, M)


def tree_that_never_leaves(n, M, K, seed, m_star, sticky, p_sticky):
    """A tree in which position m_star is rewritten by every node whose parent holds a value outside `sticky` there (to a
    sticky value with probability p_sticky) and by no node whose parent holds a sticky one: once a branch has entered the
    sticky set it never leaves it.  The root starts outside."""
    tree = plain_tree(n, M, K, seed)
    rng = np.random.default_rng(seed + 77)
    bits, vals = tree_parts(tree)
    sticky = np.asarray(sticky, dtype=bool)
    inside, outside = np.flatnonzero(sticky), np.flatnonzero(~sticky)
    root = tree["root"].copy()
    root[m_star] = outside[int(rng.integers(len(outside)))]
    cur = [int(root[m_star])] * 17
    depths = tree["depths"].tolist()
    go_in = rng.random(n) < p_sticky
    pick_in, pick_out = rng.integers(len(inside), size=n), rng.integers(len(outside), size=n)
    for i in range(1, n):
        d = depths[i]
        v = cur[d - 1]
        if sticky[v]:
            bits[i, m_star] = False
        else:
            v = int(inside[pick_in[i]] if go_in[i] else outside[pick_out[i]])
            bits[i, m_star] = True
            vals[i, m_star] = v
        cur[d] = v
    return tree_from_parts(root, tree["depths"], bits, vals, M)


# ---- classes -------------------------------------------------------------------------------------------------------------
# A class is a function (M, K, n, seed) -> dict(cb=float32 [M][K][1], queries=float32 [4][M], tree=..., T0=the table of
# the all-zero query by construction).

def _queries(cb, tree, far):
    """[zero, code a, far, code b]: a and b the codes of nodes n // 3 and (2 n) // 3."""
    from deltapq_amd import synth
    codes = synth.decode_tree_codes(tree)
    M = cb.shape[0]
    n = len(codes)
    mm = np.arange(M)
    q = np.zeros((4, M), dtype=np.float32)
    q[1] = cb[mm, codes[n // 3], 0]
    q[2] = far
    q[3] = cb[mm, codes[(2 * n) // 3], 0]
    return q


def _make(J, E, tree, far):
    cb = grid_codebook(J, E)
    return dict(cb=cb, queries=_queries(cb, tree, far), tree=tree, T0=table_by_construction(J, E))


def zero_threshold(M=8, K=256, n=N_SCAN, seed=0):
    """The query is a code that occurs often: the k-th distance is +0.0, tau' - sum of minima is 0."""
    rng = np.random.default_rng(seed)
    J = rng.integers(-2000, 2001, size=(M, K))
    tree = tree_with_copies_of_the_root(n, M, K, seed + 1, copies=24)
    out = _make(J, 0, tree, far=np.float32(5000.0))
    out["queries"][1] = out["cb"][np.arange(M), tree["root"], 0]            # the root's code: at least 25 times in the index
    return out


def constant(M=8, K=256, n=N_SCAN, seed=0):
    """Every codeword of a sub-space equal: all n distances share one bit pattern, the span of the keys is zero."""
    rng = np.random.default_rng(seed)
    J = np.repeat(rng.integers(1, 2001, size=(M, 1)), K, axis=1)
    return _make(J, 0, plain_tree(n, M, K, seed + 1), far=np.float32(-3000.0))


def ulp_crowd(M=8, K=256, n=N_SCAN, seed=0):
    """T[0][.] = 9 * 2^20, the other sub-spaces 0, 1, 4, 9 (mostly 0): the best distances are consecutive fp32 values with
    crowds of codes on each, and the filter's slack tau * 2^-20 is as wide as what it has to separate."""
    rng = np.random.default_rng(seed)
    J = rng.choice(4, size=(M, K), p=[0.8, 0.1, 0.05, 0.05])
    E = np.zeros((M, K), dtype=np.int64)
    J[0], E[0] = 3, 10
    return _make(J, E, plain_tree(n, M, K, seed + 1), far=np.float32(-1.0))


def fp32_ties(M=8, K=256, n=N_SCAN, seed=0):
    """T[0][k] = j^2 * 2^30 (j = 1, 2, 3), the other sub-spaces squares below 2^10: an fp32 ulp of the distances is 128 or
    more, so codes tie in fp32 whose exact sums differ, and the plain index's M roundings go their own way."""
    rng = np.random.default_rng(seed)
    J = rng.integers(0, 32, size=(M, K))
    E = np.zeros((M, K), dtype=np.int64)
    J[0], E[0] = rng.choice([1, 1, 1, 2, 3], size=K), 15
    return _make(J, E, plain_tree(n, M, K, seed + 1), far=np.float32(-40.0))


def _ladder(e0, far):
    def cls(M=8, K=256, n=N_SCAN, seed=0):
        rng = np.random.default_rng(seed)
        E = e0 + np.floor(25 * rng.random((M, K)) ** (M / 4)).astype(np.int64)
        return _make(np.ones((M, K), dtype=np.int64), E, plain_tree(n, M, K, seed + 1), far=np.float32(far))
    return cls


# T = 4^e, e over 25 consecutive values from e0 on: 2^-148 .. 2^-100, 2^-24 .. 2^24, 2^74 .. 2^122 (16 of the last stay below 2^128)
ladder_low = _ladder(-74, -2.0 ** -60)
ladder_low.__doc__ = "One-hot exponents from the smallest fp32 denormals up: distances, thresholds and scales below FLT_MIN."
ladder_mid = _ladder(-12, -2.0 ** 14)
ladder_mid.__doc__ = "One-hot exponents around 1: the distance bits span fifty binades."
ladder_high = _ladder(37, -2.0 ** 59)
ladder_high.__doc__ = "One-hot exponents up to 2^122: sums near FLT_MAX, none reaching 2^128; scales near FLT_MIN."


def tiny_gaussian(M=8, K=256, n=N_SCAN, seed=0):
    """A normal table on the grid 2^-74: every distance is below 2^-125, so QT / (tau' - sum of minima) exceeds FLT_MAX."""
    rng = np.random.default_rng(seed)
    J = np.clip(np.rint(rng.normal(0.0, 200.0, size=(M, K))), -4095, 4095).astype(np.int64)
    return _make(J, -74, plain_tree(n, M, K, seed + 1), far=np.float32(-2.0 ** -63))


def overflow(M=8, K=256, n=N_SCAN, seed=0):
    """Entries from 2^104 to just under 2^127, and c = 2^64 (entry +inf) for most codewords of the last sub-space, which a
    branch never leaves again: most codes are at +inf, a few dozen finite, two 2^127 entries together overflow too."""
    rng = np.random.default_rng(seed)
    J = rng.integers(1, 725, size=(M, K))
    E = np.full((M, K), 52, dtype=np.int64)
    J[0, rng.random(K) < 0.25] = 2895                 # 2895^2 * 2^104 = 2^126.998
    J[1, rng.random(K) < 0.25] = 2895
    sticky = np.arange(K) % 16 != 5                   # 15 of 16 codewords of the last sub-space are 2^64
    J[M - 1, sticky], E[M - 1, sticky] = 1, 64
    tree = tree_that_never_leaves(n, M, K, seed + 1, M - 1, sticky, p_sticky=0.85)
    cb = grid_codebook(J, E)
    T0 = table_by_construction(J, E)
    for k in np.flatnonzero(sticky):
        T0[M - 1][k] = INF                             # (float)((double)0 + 2^128)
    return dict(cb=cb, queries=_queries(cb, tree, np.float32(-2.0 ** 60)), tree=tree, T0=T0)


CLASSES = dict(zero_threshold=zero_threshold, constant=constant, ulp_crowd=ulp_crowd, fp32_ties=fp32_ties,
               ladder_low=ladder_low, ladder_mid=ladder_mid, ladder_high=ladder_high, tiny_gaussian=tiny_gaussian,
               overflow=overflow)


def build_class(name, M=8, K=256, n=N_SCAN, seed=0, n_queries=4, plain_rule=True):
    """dict(cb, queries, tree, payload, codes, tables=[[M][K] rationals per query], d64, d32 = float32 [nq][n] by the DTC and
    (plain_rule) by the plain rule).  The all-zero query's table by construction is asserted to be what the book gives."""
    from deltapq_amd import synth
    c = CLASSES[name](M, K, n, seed)
    c["name"], c["M"], c["K"], c["n"] = name, M, K, n
    c["queries"] = c["queries"][:n_queries]
    c["payload"], _ = synth.encode_dtc(c["tree"])
    c["codes"] = synth.decode_tree_codes(c["tree"])
    c["tables"] = [table_by_the_book(c["cb"], q) for q in c["queries"]]
    assert c["tables"][0] == c["T0"], "%s: the table by construction is not the table by the book" % name
    c["d64"] = np.stack([exact_distances(T, c["codes"]) for T in c["tables"]])
    if plain_rule:
        c["d32"] = np.stack([exact_distances_fp32_rule(T, c["codes"]) for T in c["tables"]])
    return c


# ---- properties: what makes a class non-vacuous, asserted on the reference alone ----------------------------------------

def kth(d, k):
    """The k-th smallest distance (no NaNs here, and no -0.0: a float sort is the sort by bits)."""
    return np.sort(d)[k - 1]


def filter_scale_exact(T, tau, QT):
    """QT / (tau' - sum of minima) in exact arithmetic, tau' = tau (1 + 2^-20); None where tau' - sum of minima is 0."""
    B = sum(min(v for v in row if v != INF) for row in T)
    R = from_f32(tau) * (1 + F(1, 2 ** 20)) - B
    return F(QT) / R if R > 0 else None


FLT_MAX = F(2) ** 128 - F(2) ** 104


def check_property(c):
    """Asserts the property row of c's class (the issue's table) on the reference."""
    name, d64, d32, n = c["name"], c["d64"], c.get("d32"), c["n"]
    bits = d64.view(np.uint32)
    if name == "zero_threshold":
        assert np.count_nonzero(bits[1] == 0) >= 20 and kth(d64[1], 10).view(np.uint32) == 0     # +0.0, at least 2 k times
    elif name == "constant":
        for q in range(len(d64)):
            assert len(np.unique(bits[q])) == 1
            assert np.array_equal(topk(d64[q], 10)[0], np.arange(10))
    elif name == "ulp_crowd":
        vals, counts = np.unique(bits[0], return_counts=True)
        assert np.all(np.diff(vals[:3].astype(np.int64)) == 1) and np.all(counts[:3] >= 16)      # consecutive fp32 values, crowded
        assert vals[0] <= kth(d64[0], 10).view(np.uint32) <= vals[2]
        for k in (10, 1000):
            tau = from_f32(kth(d64[0], k))
            assert tau * F(1, 2 ** 20) >= tau - from_f32(d64[0].min())                            # slack >= spread of the top-k
    elif name == "fp32_ties":
        units, _, g = table_units(c["tables"][0])
        tenth = kth(d64[0], 10)
        group = np.flatnonzero(d64[0] == tenth)
        sums = units[np.arange(c["M"]), c["codes"][group]].sum(axis=1)
        assert len(group) >= 4 and len(np.unique(sums)) >= 4                                      # fp32 ties, exact sums apart
        differs = [not np.array_equal(topk(d64[q], 10)[0], topk(d32[q], 10)[0]) or
                   not np.array_equal(topk(d64[q], 10)[1].view(np.uint32), topk(d32[q], 10)[1].view(np.uint32))
                   for q in range(len(d64))]
        assert any(differs)                                                                       # the two rules answer differently
    elif name.startswith("ladder"):
        top = np.sort(d64[0])[:1000]
        assert top[0] > 0 and math.log2(float(top[-1])) - math.log2(float(top[0])) >= 20         # the top-1000 span 20 binades
        if name == "ladder_low":
            assert top[0] < 2.0 ** -126 and kth(d64[0], 1) < 2.0 ** -125 and kth(d64[0], 10) < 2.0 ** -125
        if name == "ladder_high":
            assert np.all(np.isfinite(d64[0])) and sum(max(row) for row in c["tables"][0]) < F(2) ** 128
    elif name == "tiny_gaussian":
        for q in (0, 1, 3):
            for k in (1, 10, 1000):
                assert kth(d64[q], k) < 2.0 ** -125
            for QT in (64, 250):
                s = filter_scale_exact(c["tables"][q], kth(d64[q], 10), QT)
                assert s is not None and s > FLT_MAX                                              # the scale overflows fp32
    elif name == "overflow":
        finite = np.isfinite(d64[0])
        assert np.isfinite(kth(d64[0], 10)) and np.count_nonzero(~finite) >= 100 and 10 <= np.count_nonzero(finite) < 1000
        ids, d = topk(d64[0], 1000)
        tail = ~np.isfinite(d)
        assert tail.any() and np.all(ids[tail] >= 0) and np.all(np.diff(ids[tail]) > 0)           # real ids at +inf, by id
        _, is_inf, _ = table_units(c["tables"][0])
        assert np.any(~finite & ~is_inf[np.arange(c["M"]), c["codes"]].any(axis=1))               # a SUM of finite entries overflows
    else:
        raise KeyError(name)


# ---- the answers -----------------------------------------------------------------------------------------------------------

def topk(d, k, mask=None):
    """(ids int32 [k], dists float32 [k]) of one query: by (distance bits, id), over the codes `mask` (bool over ids) allows;
    padded with -1 / +inf.  n is odd in every case here, so a reported id is a position."""
    import _option_matrix as om
    pos = np.arange(len(d), dtype=np.int64)
    if mask is not None:
        ok = pos < len(mask)
        ok[ok] = mask[pos[ok]]
        pos = pos[ok]
    return om.topk_row(d, pos, pos, k)


def range_list(d, r):
    """(ids, dists) with d < r strictly, by (distance bits, id); r = +inf: every code, the +inf ones included
    (include/deltapq_amd.h: "+inf every code of the handle")."""
    pos = np.arange(len(d)) if np.isposinf(r) else np.flatnonzero(d < np.float32(r))
    pos = pos[np.lexsort((pos, d[pos].view(np.uint32)))]
    return pos.astype(np.int32), d[pos]


# ---- paths -----------------------------------------------------------------------------------------------------------------
# name -> dict(opts: open options, n, nqs: batch sizes of the calls, M, plain: open_plain, proof: profile counter -> "pos" / 0
# after the first unfiltered call of every batch size).  n is the smallest size at which the path exists: 4097 is two
# scan workgroups' worth of segments and more than one tile; bootstrap = 1 takes 16 K nodes per shard, and
# DPQ_OPT_FORCE_STRANDS a bootstrap shard (tests/_option_matrix.py uses the same 17 001).

def _path(opts, n, nqs, proof, M=8, plain=False):
    return dict(opts=opts, n=n, nqs=nqs, proof=proof, M=M, plain=plain)


_SCAN_PROOF = dict(scan_launches="pos", bootstrap_launches=0, stream_launches=0, strand_launches=0, strand1_launches=0)
_SCAN = dict(bootstrap=-1, batch_decode=-1, stream_max_queries=-1)
PATHS = {
    "scan_decode_in_scan": _path(_SCAN, N_SCAN, (33,), _SCAN_PROOF),
    "scan_no_tighten": _path(dict(_SCAN, flags=16), N_SCAN, (33,), _SCAN_PROOF),
    "scan_after_bootstrap": _path(dict(bootstrap=1), N_BOOT, (33,), dict(bootstrap_launches="pos", scan_launches="pos")),
    "scan_after_bootstrap_quantise_kernel": _path(dict(bootstrap=1, flags=2), N_BOOT, (33,),
                                                  dict(bootstrap_launches="pos", quantise_ms="pos")),
    "scratch_labels": _path(dict(batch_decode=1), N_SCAN, (65,), dict(decode_ms="pos", scan_launches="pos")),
    "scratch_no_labels": _path(dict(batch_decode=1, flags=1), N_SCAN, (65,), dict(decode_ms="pos", scan_launches="pos")),
    "stream": _path(dict(bootstrap=-1), N_SCAN, (1, 2, 4), dict(stream_launches="pos", strand_launches=0, strand1_launches=0)),
    "strand": _path(dict(bootstrap=1, flags=64), N_BOOT, (2, 4), dict(strand_launches="pos", strand1_launches=0)),
    "strand1": _path(dict(bootstrap=1, flags=64), N_BOOT, (1,), dict(strand1_launches="pos")),
    "strand_one_query_exact_tables": _path(dict(bootstrap=1, flags=192), N_BOOT, (1,), dict(strand_launches="pos", strand1_launches=0)),
    "m16_scan": _path(_SCAN, N_SCAN, (33,), _SCAN_PROOF, M=16),
    "m16_stream": _path(dict(bootstrap=-1), N_SCAN, (1,), dict(stream_launches="pos", strand_launches=0, strand1_launches=0), M=16),
    "plain_index_fp32_rule": _path(dict(bootstrap=-1), N_SCAN, (33,), dict(scan_launches="pos"), plain=True),
}


def check_proof(prof, proof, what):
    for name, want in proof.items():
        if want == "pos":
            assert prof[name] > 0, "%s: %s = %r, the path did not run" % (what, name, prof[name])
        else:
            assert prof[name] == want, "%s: %s = %r, another kernel ran" % (what, name, prof[name])


def half_mask(n, seed):
    return np.random.default_rng(seed).random(n) < 0.5


def run_path(api, oracle, c, path, what):
    """One handle, every call of the issue's list, each strictly against the exact reference of c (build_class at the
    path's n and M); the unfiltered answers also tie-aware against the oracle."""
    import _option_matrix as om
    from oracle.dtc_oracle import tie_aware_equal
    n, M, K = c["n"], c["M"], c["K"]
    assert (n, M) == (path["n"], path["M"]) and n % 2 == 1
    alld = c["d32"] if path["plain"] else c["d64"]
    U = len(c["queries"])
    luts = [np_table(T) for T in c["tables"]]

    def oracle_row(u, k):
        if path["plain"]:
            return oracle.pqscan_plain(c["codes"], luts[u], k)
        return oracle.scan_lut(c["payload"], n, luts[u], k)

    if path["plain"]:
        idx = api.DeltaPQIndex.open_plain(c["codes"], K=K, **path["opts"])
    else:
        idx = api.DeltaPQIndex.open_memory(c["payload"], n, M, K, **path["opts"])
    with idx:
        idx.set_codebook(c["cb"])
        idx.profile_enable(True)
        mask = half_mask(n, 12345)
        for nq in path["nqs"]:
            use = np.arange(nq) % U
            qs = np.ascontiguousarray(c["queries"][use])
            w = "%s nq=%d" % (what, nq)
            # top-k at k = 10, with the proof that the named kernel answered it
            idx.profile_reset()
            got = idx.query_batch(qs, 10)
            check_proof(idx.profile_read(), path["proof"], w)
            om._rows_equal(got, [topk(alld[u], 10) for u in use], w + " top-10")
            for q, u in enumerate(use[:U]):
                oi, od = oracle_row(u, 10)
                ok, msg = tie_aware_equal(got[0][q], got[1][q], oi, od, alld[u], n)
                assert ok, "%s query %d against the oracle: %s" % (w, q, msg)
            # k = 1 and k = 1000
            for k in (1, 1000):
                om._rows_equal(idx.query_batch(qs, k), [topk(alld[u], k) for u in use], "%s top-%d" % (w, k))
            # range search: nextafter of the 10th distance, and the 10th distance itself (strict <: without its tie group)
            tenth = np.array([kth(alld[u], 10) for u in use], dtype=np.float32)
            for r, kind in ((np.nextafter(tenth, np.float32(np.inf)), "nextafter of the 10th distance"), (tenth, "the 10th distance")):
                om._range_equal(idx.range_search(qs, r), [range_list(alld[u], r[q]) for q, u in enumerate(use)],
                                "%s range (%s)" % (w, kind))
            if c["name"] == "overflow":
                r = np.full(nq, np.inf, dtype=np.float32)
                om._range_equal(idx.range_search(qs, r), [range_list(alld[u], np.inf) for u in use], w + " range (+inf)")
            # filtered top-k under a half-density mask
            with api.IdFilter.from_mask(idx, mask) as f:
                got = idx.query_batch_filtered(qs, 10, f)
            om._rows_equal(got, [topk(alld[u], 10, mask) for u in use], w + " filtered top-10")
