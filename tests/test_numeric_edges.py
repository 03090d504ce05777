"""Every scan path on distance tables at the numeric edges (tests/_numeric_edges.py): zero span, zero threshold, a threshold a
few ulps above the sum of the minima, fp32 ties with different exact sums, distance bits over fifty binades, scales beyond
FLT_MAX and near FLT_MIN, +inf entries and sums.

CPU: the rounding helper against numpy; every class's property (what makes it non-vacuous) on the exact-rational reference
alone; the oracle, its Python restatement and the reference agree on the fp32 bits of every code, for both distance rules.
GPU: class x path, each case one open handle whose answers -- top-k at k = 1, 10, 1000, filtered top-k, range search at two
radii -- are compared strictly (ids and distance bits) with the reference, after the profile counters have shown that the
path's kernel is the one that answered.
"""
import numpy as np
import pytest

import _numeric_edges as ne
from _numeric_edges import F, INF

# (M, n) of the paths
COMBOS = [(8, ne.N_SCAN), (8, ne.N_BOOT), (16, ne.N_SCAN)]
_cache = {}


def built_class(name, M, n):
    """One build per (class, M, n) and module; nobody writes to it."""
    key = (name, M, n)
    if key not in _cache:
        _cache[key] = ne.build_class(name, M, 256, n, plain_rule=(M, n) == (8, ne.N_SCAN))
    return _cache[key]


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


# ---- the rounding helper ------------------------------------------------------------------------------------------------

def test_rounding_helper_agrees_with_numpy():
    rng = np.random.default_rng(0)
    vals = []
    # doubles all over fp32's range and beyond both ends
    vals += list(np.ldexp(rng.uniform(1.0, 2.0, 3000), rng.integers(-160, 131, 3000)) * rng.choice([-1.0, 1.0], 3000))
    # the denormal range, densely
    vals += list(np.ldexp(rng.uniform(0.0, 1.0, 1000), rng.integers(-152, -124, 1000)))
    # halfway cases: the midpoint of two neighbouring fp32 values (a double), and its two double neighbours
    a = np.concatenate([rng.integers(0, 0x7f7fffff, 1000, dtype=np.int64), np.arange(0, 40), np.arange(0x007ffff0, 0x00800010),
                        np.arange(0x7f7ffff0, 0x7f7fffff)]).astype(np.uint32)
    lo, hi = a.view(np.float32).astype(np.float64), (a + np.uint32(1)).view(np.float32).astype(np.float64)
    mid = lo + (hi - lo) / 2
    vals += list(mid) + list(np.nextafter(mid, 0.0)) + list(np.nextafter(mid, np.inf))
    # the overflow edge: FLT_MAX, the tie at 2^128 - 2^103 (to even: +inf) and its neighbours, 2^128
    top = 2.0 ** 128 - 2.0 ** 103
    vals += [float(np.finfo(np.float32).max), top, float(np.nextafter(top, 0.0)), float(np.nextafter(top, np.inf)), 2.0 ** 128,
             -top, 0.0, 2.0 ** -149, 2.0 ** -150, float(np.nextafter(2.0 ** -150, 1.0)), 2.0 ** -126, 1.5 * 2.0 ** -149]
    assert len(vals) > 7000
    with np.errstate(over="ignore", under="ignore"):
        want = np.asarray(vals, dtype=np.float64).astype(np.float32)
    for v, w in zip(vals, want):
        got = ne.rne32(F(float(v)))
        if np.isinf(w):
            assert got == (INF if w > 0 else -INF), v
        else:
            assert got == F(float(w)), (v, got, w)
            assert ne.to_f32(got).view(np.uint32) == w.view(np.uint32) or w == 0      # (-0.0 has no rational)
    # 53 bits: Python's own correctly rounded int / int
    for _ in range(2000):
        x = F(int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62)))
        assert ne.rne64(x) == F(x.numerator / x.denominator)
    assert ne.rne64(F(2) ** 1024 - F(2) ** 970) == INF and ne.rne64(F(1, 2 ** 1075)) == 0 and ne.rne64(F(3, 2 ** 1075)) == F(1, 2 ** 1073)


# ---- the classes, on the CPU ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,n", COMBOS, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(ne.CLASSES))
def test_class_property_and_oracle_agree_with_the_exact_reference(oracle, name, M, n):
    """The class has the property that makes it an edge (on the reference alone), and for every query the oracle's table,
    its incremental fp64 stack and its fp32 plain scan give exactly the reference's bits for every code."""
    if name == "fp32_ties" and (M, n) != (8, ne.N_SCAN):
        c = ne.build_class(name, M, 256, n)                  # (its property compares the two rules)
    else:
        c = built_class(name, M, n)
    ne.check_property(c)
    for u, q in enumerate(c["queries"]):
        lut = oracle.build_lut(c["cb"], q)
        assert np.array_equal(lut.view(np.uint32), ne.np_table(c["tables"][u]).view(np.uint32)), "query %d: tables differ" % u
        alld = oracle.scan_lut(c["payload"], n, lut, 1, want_all=True)[2]
        assert np.array_equal(alld.view(np.uint32), c["d64"][u].view(np.uint32)), "query %d: the fp64 stack differs" % u
        if "d32" in c:
            ids, d = oracle.pqscan_plain(c["codes"], lut, n)
            assert np.array_equal(np.sort(ids), np.arange(n)), "query %d: the plain scan's ids" % u
            assert np.array_equal(d.view(np.uint32), c["d32"][u][ids].view(np.uint32)), "query %d: the fp32 rule differs" % u
            assert np.all(np.diff(d.view(np.uint32).astype(np.int64)) >= 0)


@pytest.mark.parametrize("name", list(ne.CLASSES))
def test_python_restatement_agrees_with_the_exact_reference(name):
    """oracle/dtc_oracle.py's py_build_lut and py_scan (M = 8 streams, small n: it is slow) on the first codes of the class."""
    from deltapq_amd import synth
    from oracle import dtc_oracle as O
    import _option_matrix as om
    c = built_class(name, 8, ne.N_SCAN)
    n = ne.SMALL_N
    payload, _ = synth.encode_dtc(om.sub_tree(c["tree"], n))
    for u, q in enumerate(c["queries"]):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            lut = np.asarray(O.py_build_lut(c["cb"], q), dtype=np.float32)
            alld = O.py_scan(payload, n, lut, 1)[2]
        assert np.array_equal(lut.view(np.uint32), ne.np_table(c["tables"][u]).view(np.uint32)), "query %d: tables differ" % u
        assert np.array_equal(alld.view(np.uint32), c["d64"][u][:n].view(np.uint32)), "query %d: distances differ" % u


def test_paths_cover_the_table_of_the_issue():
    assert len(ne.PATHS) == 13 and {(p["M"], p["n"]) for p in ne.PATHS.values()} == set(COMBOS)
    assert all(p["n"] % 2 == 1 and p["n"] > 1000 for p in ne.PATHS.values())       # odd N: ids are positions; k = 1000 fits


# ---- class x path on the GPU ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", list(ne.PATHS))
@pytest.mark.parametrize("name", list(ne.CLASSES))
def test_numeric_edge_on_path(gpu, oracle, name, path):
    p = ne.PATHS[path]
    ne.run_path(gpu, oracle, built_class(name, p["M"], p["n"]), p, "%s on %s" % (name, path))
