"""Search by caller-supplied distance tables (dpq_query_batch_tables, dpq_query_batch_device_tables,
dpq_range_search_tables): the engine answers from tables[nq][M][K] what it answers from queries whose L2 tables those are.

GPU: every scan path on exact tables without a codebook, strictly (ids and distance bits) against the exact-rational
reference of tests/_numeric_edges.py; every mandatory case of the option matrix, tables == queries; the state a table call
leaves behind; bad and degenerate entries.  CPU: dpq_ip_scores, the argument checks, the restatement's own properties.
"""
import ctypes

import numpy as np
import pytest

import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as R

ERR_ARG = -1
_cache = {}


def built_class(name, M, n):
    """One build per (class, M, n) and module; nobody writes to it."""
    key = (name, M, n)
    if key not in _cache:
        _cache[key] = ne.build_class(name, M, 256, n, plain_rule=(M, n) == (8, ne.N_SCAN))
        _cache[key]["luts"] = np.stack([ne.np_table(T) for T in _cache[key]["tables"]])
    return _cache[key]


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Two answers (top-k pairs or range triples) equal: integers exactly, floats to the bit."""
    return len(a) == len(b) and all(np.array_equal(x, y) if x.dtype.kind == "i" else np.array_equal(bits(x), bits(y))
                                    for x, y in zip(a, b))


# ---- 1. every scan path, exact tables, no codebook ---------------------------------------------------------------------

def _table_calls(api, idx, c, path, what, proof):
    """Every table call of the issue's list on one handle, each strictly against the exact reference; returns the answers."""
    n = c["n"]
    alld = c["d32"] if path["plain"] else c["d64"]
    U = len(c["queries"])
    mask = ne.half_mask(n, 12345)
    out = []
    for nq in path["nqs"]:
        use = np.arange(nq) % U
        tabs = np.ascontiguousarray(c["luts"][use])
        w = "%s nq=%d" % (what, nq)
        idx.profile_reset()
        got = idx.query_batch_tables(tabs, 10)
        if proof:
            ne.check_proof(idx.profile_read(), path["proof"], w)
        om._rows_equal(got, [ne.topk(alld[u], 10) for u in use], w + " top-10")
        out.append(got)
        for k in (1, 1000):
            got = idx.query_batch_tables(tabs, k)
            om._rows_equal(got, [ne.topk(alld[u], k) for u in use], "%s top-%d" % (w, k))
            out.append(got)
        tenth = np.array([ne.kth(alld[u], 10) for u in use], dtype=np.float32)
        radii = [(tenth, "the 10th distance"), (np.nextafter(tenth, np.float32(np.inf)), "nextafter of the 10th distance")]
        if c["name"] == "overflow":
            radii.append((np.full(nq, np.inf, dtype=np.float32), "+inf"))
        for r, kind in radii:
            got = idx.range_search_tables(tabs, r)
            om._range_equal(got, [ne.range_list(alld[u], r[q]) for q, u in enumerate(use)], "%s range (%s)" % (w, kind))
            out.append(got)
        with api.IdFilter.from_mask(idx, mask) as f:
            got = idx.query_batch_tables(tabs, 10, id_filter=f)
        om._rows_equal(got, [ne.topk(alld[u], 10, mask) for u in use], w + " filtered top-10")
        out.append(got)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(ne.PATHS))
@pytest.mark.parametrize("name", ["fp32_ties", "overflow"])
def test_tables_on_every_scan_path(gpu, name, path):
    """fp32_ties separates the DTC rule from the plain rule, overflow carries +inf entries; both classes have a plain rule
    at the plain path's size, so nothing is skipped."""
    p = ne.PATHS[path]
    c = built_class(name, p["M"], p["n"])
    assert not p["plain"] or "d32" in c
    what = "%s tables on %s" % (name, path)
    if p["plain"]:
        idx = gpu.DeltaPQIndex.open_plain(c["codes"], K=c["K"], **p["opts"])
    else:
        idx = gpu.DeltaPQIndex.open_memory(c["payload"], c["n"], c["M"], c["K"], **p["opts"])
    with idx:
        idx.profile_enable(True)
        before = _table_calls(gpu, idx, c, p, what + " (no codebook)", proof=True)
        idx.set_codebook(c["cb"])
        after = _table_calls(gpu, idx, c, p, what + " (codebook set)", proof=False)
        assert len(before) == len(after) and all(same(a, b) for a, b in zip(before, after)), \
            what + ": the answers changed with dpq_set_codebook"
        U = len(c["queries"])
        for nq in p["nqs"]:
            use = np.arange(nq) % U
            by_q = idx.query_batch(np.ascontiguousarray(c["queries"][use]), 10)
            by_t = idx.query_batch_tables(np.ascontiguousarray(c["luts"][use]), 10)
            assert same(by_q, by_t), "%s nq=%d: query_batch(queries) differs from query_batch_tables(tables)" % (what, nq)


# ---- 2. every open option: tables == queries -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", om.MANDATORY, ids=om.case_id)
def test_tables_equal_queries_on_every_open_option(gpu, oracle, case):
    from deltapq_amd.dist import merge_range_host
    c = case
    what = om.case_id(c)
    inp = om.build_inputs(c)
    alld = om.oracle_distances(oracle, c, inp)
    tabs = R.l2_tables(inp["cb"], inp["qs"])
    for q in range(c["nq"]):
        lut = oracle.build_lut(inp["cb"], inp["qs"][q])
        assert np.array_equal(bits(lut)[:, :c["K"]], bits(tabs[q])), "%s query %d: the restated L2 table is not the oracle's" % (what, q)
    masks = [m for m in om.make_masks(c) if m[0] in ("ones", "random")]
    rnd = dict(masks)["random"]
    radii = om.radii_calls(c, alld)[:1]
    k, qs = om.call_k(c), inp["qs"]
    parts = []
    for rank in range(c["shards"]):
        w = what if c["shards"] == 1 else "%s rank %d" % (what, rank)
        with gpu.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c, rank)) as idx:
            idx.set_codebook(inp["cb"])
            info = idx.info()
            ref = om.handle_reference(c, alld, masks, radii, info["node_lo"], info["node_hi"])
            top_t, top_q = idx.query_batch_tables(tabs, k), idx.query_batch(qs, k)
            assert same(top_t, top_q), w + ": top-k by tables differs from top-k by queries"
            om._rows_equal(top_t, ref["filtered"]["ones"][1], w + " top-k by tables")
            with gpu.IdFilter.from_mask(idx, rnd) as f:
                fil_t, fil_q = idx.query_batch_tables(tabs, k, id_filter=f), idx.query_batch_filtered(qs, k, f)
            assert same(fil_t, fil_q), w + ": filtered top-k by tables differs from filtered top-k by queries"
            om._rows_equal(fil_t, ref["filtered"]["random"][1], w + " filtered top-k by tables")
            rng_t, rng_q = idx.range_search_tables(tabs, radii[0]), idx.range_search(qs, radii[0])
            assert same(rng_t, rng_q), w + ": range search by tables differs from range search by queries"
            om._range_equal(rng_t, ref["ranges"][0], w + " range search by tables")
            parts.append((top_t, fil_t, rng_t))
    if c["shards"] > 1:
        whole = om.handle_reference(c, alld, masks, radii, None, None)
        for j, name in enumerate(("ones", "random")):
            merged = gpu.merge_topk_host(np.stack([p[j][0] for p in parts]), np.stack([p[j][1] for p in parts]))
            om._rows_equal(merged, whole["filtered"][name][1], "%s merged top-k by tables (%s)" % (what, name))
        om._range_equal(merge_range_host([p[2] for p in parts]), whole["ranges"][0], what + " merged range search by tables")


# ---- 3. state --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,nq,opts", [(ne.N_SCAN, 65, dict(batch_decode=1)), (ne.N_BOOT, 1, dict(bootstrap=1, flags=64))],
                         ids=["scratch_nq65", "strand1_nq1"])
def test_table_calls_leave_the_handle_as_they_found_it(gpu, n, nq, opts):
    """query_batch -> query_batch_tables (other tables) -> query_batch -> range_search_tables -> query_batch_tables: every
    answer right, the two query_batch answers equal to the bit.  A clear the ingest kernel missed shows here."""
    c = built_class("fp32_ties", 8, n)
    alld, U = c["d64"], len(c["queries"])
    use = np.arange(nq) % U
    other = (use + 1) % U                       # the table call asks each slot about ANOTHER query of the class
    qs, tabs = np.ascontiguousarray(c["queries"][use]), np.ascontiguousarray(c["luts"][other])
    want_q = [ne.topk(alld[u], 10) for u in use]
    want_t = [ne.topk(alld[u], 10) for u in other]
    tenth = np.array([ne.kth(alld[u], 10) for u in other], dtype=np.float32)
    with gpu.DeltaPQIndex.open_memory(c["payload"], n, 8, 256, **opts) as idx:
        idx.set_codebook(c["cb"])
        first = idx.query_batch(qs, 10)
        om._rows_equal(first, want_q, "query_batch, first")
        om._rows_equal(idx.query_batch_tables(tabs, 10), want_t, "query_batch_tables, first")
        again = idx.query_batch(qs, 10)
        om._rows_equal(again, want_q, "query_batch after a table call")
        assert same(first, again)
        om._range_equal(idx.range_search_tables(tabs, tenth), [ne.range_list(alld[u], tenth[q]) for q, u in enumerate(other)],
                        "range_search_tables")
        om._rows_equal(idx.query_batch_tables(tabs, 10), want_t, "query_batch_tables after a range call")
        om._rows_equal(idx.query_batch(qs, 10), want_q, "query_batch, last")


# ---- 4. bad entries ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("-inf")], ids=["negative", "nan", "minus_inf"])
def test_bad_entry_is_an_argument_error(gpu, bad):
    """nq = 5, the bad entry in query 3: DPQ_ERR_ARG from the host form (checked on the host) and from the device form (the
    ingest kernel's flag, read back); the handle then answers a query call to the bit."""
    import torch
    c = built_class("fp32_ties", 8, ne.N_SCAN)
    alld, U = c["d64"], len(c["queries"])
    use = np.arange(5) % U
    qs, tabs = np.ascontiguousarray(c["queries"][use]), np.ascontiguousarray(c["luts"][use])
    tabs[3, 2, 17] = bad
    with gpu.DeltaPQIndex.open_memory(c["payload"], c["n"], 8, 256) as idx:
        idx.set_codebook(c["cb"])
        with pytest.raises(gpu.DpqError) as e:
            idx.query_batch_tables(tabs, 10)
        assert e.value.status == ERR_ARG
        with pytest.raises(gpu.DpqError) as e:
            idx.range_search_tables(tabs, 1.0)
        assert e.value.status == ERR_ARG
        with pytest.raises(gpu.DpqError) as e:
            idx.query_batch_tables_torch(torch.from_numpy(tabs).cuda(), 10)
        assert e.value.status == ERR_ARG
        om._rows_equal(idx.query_batch(qs, 10), [ne.topk(alld[u], 10) for u in use], "query_batch after a refused table call")
        good = np.ascontiguousarray(c["luts"][use])
        om._rows_equal(idx.query_batch_tables(good, 10), [ne.topk(alld[u], 10) for u in use], "tables after a refused call")


@pytest.mark.gpu
def test_minus_zero_is_read_as_plus_zero(gpu):
    import torch
    c = built_class("fp32_ties", 8, ne.N_SCAN)
    alld, U = c["d64"], len(c["queries"])
    use = np.arange(5) % U
    tabs = np.ascontiguousarray(c["luts"][use])
    zeros = tabs == 0
    assert zeros.any()
    tabs[zeros] = -0.0
    assert np.signbit(tabs).sum() == zeros.sum()
    want = [ne.topk(alld[u], 10) for u in use]
    with gpu.DeltaPQIndex.open_memory(c["payload"], c["n"], 8, 256) as idx:
        om._rows_equal(idx.query_batch_tables(tabs, 10), want, "host form")
        ids, d = idx.query_batch_tables_torch(torch.from_numpy(tabs).cuda(), 10)
        om._rows_equal((ids.cpu().numpy(), d.cpu().numpy()), want, "device form")


# ---- 5. degenerate tables ------------------------------------------------------------------------------------------------

def _expected(table_rows, codes, k, N):
    """Top-k rows over all codes of a DTC index of N codes (even-N rule) for one table per row."""
    pos = np.arange(len(codes), dtype=np.int64)
    rep = om.reported_ids(pos, 0, N)
    return [om.topk_row(R.distances_dtc(t, codes), pos, rep, k) for t in table_rows]


@pytest.mark.gpu
def test_degenerate_tables(gpu):
    from deltapq_amd import synth
    # all-zero tables on an even index whose every code is asked for: ids 0 .. N - 2, then N (the even-N id)
    n = 64
    tree = ne.plain_tree(n, 8, 256, seed=5)
    payload, _ = synth.encode_dtc(tree)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        ids, d = idx.query_batch_tables(np.zeros((3, 8, 256), dtype=np.float32), n)
        want = np.append(np.arange(n - 1), n).astype(np.int32)
        assert all(np.array_equal(row, want) for row in ids) and not bits(d).any()
    n = ne.N_SCAN
    tree = ne.plain_tree(n, 8, 256, seed=6, mean_diffs=1.0)
    payload, _ = synth.encode_dtc(tree)
    codes = synth.decode_tree_codes(tree)
    root = codes[n // 3]                                          # a code of the index, and its copies
    rng = np.random.default_rng(7)
    zero = np.zeros((5, 8, 256), dtype=np.float32)
    inf_row = rng.integers(0, 64, size=(5, 8, 256)).astype(np.float32)
    inf_row[:, 3, :] = np.inf                                     # one sub-space all +inf: every distance is +inf
    one_col = np.full((5, 8, 256), np.inf, dtype=np.float32)      # one finite column per row: that code's copies alone are finite
    for q in range(5):
        one_col[q, np.arange(8), root] = np.float32(q + 1)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        for name, tabs in (("all zero", zero), ("a row of +inf", inf_row), ("one finite column per row", one_col)):
            for k in (10, 100):
                om._rows_equal(idx.query_batch_tables(tabs, k), _expected(tabs, codes, k, n), "%s top-%d" % (name, k))
        ids, _ = idx.query_batch_tables(zero, 10)
        assert all(np.array_equal(row, np.arange(10)) for row in ids)
        finite = np.count_nonzero((codes == root).all(axis=1))
        assert 1 <= finite < 1000
        _, d = idx.query_batch_tables(one_col, 1000)
        assert np.all(np.isfinite(d[:, :finite])) and np.all(np.isposinf(d[:, finite:]))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------

TABLE_SYMBOLS = ("dpq_query_batch_tables", "dpq_query_batch_device_tables", "dpq_range_search_tables", "dpq_ip_tables",
                 "dpq_ip_tables_device", "dpq_query_batch_ip", "dpq_query_batch_device_ip", "dpq_ip_scores")


def test_ip_scores_against_numpy(lib):
    from deltapq_amd import api
    rng = np.random.default_rng(3)
    nq, k = 7, 33
    bias = rng.normal(0, 1e4, nq).astype(np.float32)
    gaps = np.abs(rng.normal(0, 1e3, (nq, k))).astype(np.float32)
    ids = rng.integers(0, 1000, (nq, k)).astype(np.int32)
    gaps[2, 5] = np.inf                      # a real id at +inf
    ids[4, 20:], gaps[4, 20:] = -1, np.inf   # padding
    ids[6, :], gaps[6, :] = -1, np.inf
    gaps[0, 0] = 0.0
    got = api.ip_scores(bias, gaps, ids)
    want = R.ip_scores(bias, gaps, ids)
    assert np.array_equal(bits(got), bits(want))
    assert np.isneginf(got[4, 20:]).all() and np.isneginf(got[6]).all() and np.isneginf(got[2, 5])
    assert got[0, 0] == bias[0]


def test_table_entry_points_refuse_bad_arguments_without_a_device(lib):
    from deltapq_amd import _lib
    names = {name for name, _, _ in _lib.SYMBOLS}
    assert all(name in names for name in TABLE_SYMBOLS)
    buf = np.zeros(8 * 256 * 4, dtype=np.float32)
    ib = np.zeros(64, dtype=np.int32)
    p, ip = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ib.ctypes.data)
    out = ctypes.c_void_p(1)
    # a NULL handle, whatever else is passed
    assert lib.dpq_query_batch_tables(None, None, p, 1, 1, ip, p) == ERR_ARG
    assert lib.dpq_query_batch_tables(None, None, p, -1, 1, ip, p) == ERR_ARG
    assert lib.dpq_query_batch_tables(None, None, p, 1, 0, ip, p) == ERR_ARG
    assert lib.dpq_query_batch_tables(None, None, None, 1, 1, None, None) == ERR_ARG
    assert lib.dpq_query_batch_device_tables(None, None, p, 1, 1, ip, p, None) == ERR_ARG
    assert lib.dpq_query_batch_device_tables(None, None, None, -1, 0, None, None, None) == ERR_ARG
    assert lib.dpq_range_search_tables(None, p, 1, p, ctypes.byref(out)) == ERR_ARG
    assert out.value is None                       # *out is cleared whenever it can be
    assert lib.dpq_range_search_tables(None, p, 1, p, None) == ERR_ARG
    assert lib.dpq_range_search_tables(None, None, -1, None, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_ip_tables(None, p, 1, p, p) == ERR_ARG
    assert lib.dpq_ip_tables(None, None, -1, None, None) == ERR_ARG
    assert lib.dpq_ip_tables_device(None, p, 1, p, p, None) == ERR_ARG
    assert lib.dpq_ip_tables_device(None, None, -1, None, None, None) == ERR_ARG
    assert lib.dpq_query_batch_ip(None, None, p, 1, 1, ip, p, None, None) == ERR_ARG
    assert lib.dpq_query_batch_ip(None, None, p, 1, 0, ip, p, p, p) == ERR_ARG
    assert lib.dpq_query_batch_ip(None, None, None, -1, 1, None, None, None, None) == ERR_ARG
    assert lib.dpq_query_batch_device_ip(None, None, p, 1, 1, ip, p, None, None, None) == ERR_ARG
    assert lib.dpq_query_batch_device_ip(None, None, None, -1, 0, None, None, None, None, None) == ERR_ARG
    # dpq_ip_scores has no handle: every argument is checked
    assert lib.dpq_ip_scores(p, p, ip, 2, 4, p) == 0
    assert lib.dpq_ip_scores(None, p, ip, 2, 4, p) == ERR_ARG
    assert lib.dpq_ip_scores(p, None, ip, 2, 4, p) == ERR_ARG
    assert lib.dpq_ip_scores(p, p, None, 2, 4, p) == ERR_ARG
    assert lib.dpq_ip_scores(p, p, ip, 2, 4, None) == ERR_ARG
    assert lib.dpq_ip_scores(p, p, ip, -1, 4, p) == ERR_ARG
    assert lib.dpq_ip_scores(p, p, ip, 2, 0, p) == ERR_ARG
    assert lib.dpq_ip_scores(p, p, ip, 0, 4, p) == 0


def test_restated_ip_tables_are_gaps_to_the_first_maximum():
    from deltapq_amd import synth
    for M, K, Ds in ((8, 256, 16), (16, 64, 8), (8, 17, 16), (8, 200, 5), (8, 256, 1)):
        cb = synth.make_codebook(M, K, Ds, seed=1)
        qs = synth.make_queries(9, M * Ds, seed=2)
        qs[1::2] *= -1
        p, top, e, B = R.ip_tables(cb, qs)
        assert e.shape == (9, M, K) and e.dtype == np.float32 and B.shape == (9,)
        assert np.all(e >= 0) and not np.signbit(e).any()
        first = p.argmax(axis=2)                                            # numpy: the first maximum
        assert not bits(np.take_along_axis(e, first[:, :, None], axis=2)).any()
        assert np.array_equal(np.take_along_axis(p, first[:, :, None], axis=2)[:, :, 0], top)


def test_restated_gap_order_is_the_inner_product_order_on_grid_inputs():
    """Codebook and queries as integers in -15 .. 15 times a power of two: every product, dot product, maximum, gap and
    sum is an exact integer multiple of that power, so the order by (gap, id) must be the order by exact integer inner
    product descending, ties by id."""
    rng = np.random.default_rng(11)
    M, K, Ds, n, nq = 8, 64, 4, 3000, 6
    scale_c, scale_q = 2.0 ** -3, 2.0 ** 5
    ci, qi = rng.integers(-15, 16, (M, K, Ds)), rng.integers(-15, 16, (nq, M * Ds))
    cb, qs = (ci * scale_c).astype(np.float32), (qi * scale_q).astype(np.float32)
    codes = rng.integers(0, K, (n, M))
    codes[100:140] = codes[7]                                               # ties: equal codes at different ids
    p, top, e, B = R.ip_tables(cb, qs)
    for q in range(nq):
        exact = np.zeros(n, dtype=np.int64)                                 # the integer inner product of every code
        for m in range(M):
            exact += (ci[m, codes[:, m]] * qi[q, m * Ds:(m + 1) * Ds][None, :]).sum(axis=1)
        g = R.distances_dtc(e[q], codes)
        by_gap = np.lexsort((np.arange(n), bits(g)))
        by_ip = np.lexsort((np.arange(n), -exact))
        assert np.array_equal(by_gap, by_ip)
        s = R.ip_scores(B[q:q + 1], g[None, :], np.zeros((1, n), dtype=np.int32))[0]
        assert np.array_equal(s.astype(np.float64), exact * (scale_c * scale_q))   # and the score IS the inner product
