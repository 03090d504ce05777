"""Inner-product search (dpq_ip_tables, dpq_query_batch_ip, dpq_ip_scores) against the numpy restatement of its rules
(tests/_tables_restatement.py): tables and bias bit for bit; ids, gaps, scores and bias of the search strictly; and a sanity
bound against plain float64 dot products of the codes the index itself returns.

Every table a strict check relies on is asserted exact in the sense of include/deltapq_amd.h (table_units of
tests/_numeric_edges.py): its fp64 sums round nowhere, so the gaps are defined to the bit on every scan path.
"""
import numpy as np
import pytest

import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as R

SHAPES = [(8, 256, 16), (16, 64, 8), (8, 17, 16), (8, 200, 5), (8, 256, 1)]
_cache = {}


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signed_queries(nq, D, seed):
    """synth.make_queries with every other query negated: dot products of both signs."""
    from deltapq_amd import synth
    qs = synth.make_queries(nq, D, seed)
    qs[1::2] *= -1
    return qs


def assert_exact(e, what):
    """table_units on every query's table: whole multiples of one power of two, maxima adding up to less than 2^53 units."""
    for q, table in enumerate(e):
        try:
            ne.table_units([[ne.from_f32(v) for v in row] for row in table])
        except AssertionError as err:
            raise AssertionError("%s query %d: the table is not exact: %s" % (what, q, err))


def inputs(M, K, Ds, n, nq, seed):
    """dict(cb, qs, tree, payload, codes, p, top, e, B) of a seeded index, its restated inner-product tables asserted exact."""
    key = (M, K, Ds, n, nq, seed)
    if key not in _cache:
        from deltapq_amd import synth
        cb = synth.make_codebook(M, K, Ds, seed)
        tree = ne.plain_tree(n, M, K, seed + 1)
        payload, _ = synth.encode_dtc(tree)
        qs = signed_queries(nq, M * Ds, seed + 2)
        p, top, e, B = R.ip_tables(cb, qs)
        assert_exact(e, "M=%d K=%d Ds=%d seed=%d" % (M, K, Ds, seed))
        _cache[key] = dict(cb=cb, qs=qs, tree=tree, payload=payload, codes=synth.decode_tree_codes(tree), p=p, top=top, e=e, B=B)
    return _cache[key]


def expected(inp, k, mask=None, plain=False, lo=0, hi=None):
    """(ids [nq][k], gaps, scores) by the rules: per-code gaps from the decoded codes, order by (gap bits, id), scores from
    the formula; over nodes [lo, hi) that `mask` allows.  n is odd here: ids are positions."""
    codes = inp["codes"]
    hi = len(codes) if hi is None else hi
    ok = np.zeros(len(codes), dtype=bool)
    ok[lo:hi] = True
    if mask is not None:
        ok[:len(mask)] &= mask
        ok[len(mask):] = False
    dist = R.distances_plain if plain else R.distances_dtc
    ids, gaps = zip(*[ne.topk(dist(e, codes), k, ok) for e in inp["e"]])
    ids, gaps = np.stack(ids), np.stack(gaps)
    return ids, gaps, R.ip_scores(inp["B"], gaps, ids)


def check(got, want, B, what):
    ids, scores, gaps, bias = got
    assert np.array_equal(bits(bias), bits(B)), what + ": bias"
    assert np.array_equal(bits(gaps), bits(want[1])), what + ": gaps"
    assert np.array_equal(ids, want[0]), what + ": ids"
    assert np.array_equal(bits(scores), bits(want[2])), what + ": scores"
    real = ids >= 0
    assert np.all(np.isposinf(gaps[~real])) and np.all(np.isneginf(scores[~real])), what + ": padding"
    s = np.where(real, scores, -np.inf)
    assert np.all(s[:, :-1] >= s[:, 1:]), what + ": scores do not descend"


# ---- CPU: the tables the strict checks rely on are exact --------------------------------------------------------------------

@pytest.mark.parametrize("M,K,Ds", [s for s in SHAPES if s[2] > 1], ids=str)
def test_restated_ip_tables_of_the_synthetic_inputs_are_exact(M, K, Ds):
    """Seeds 1-3, queries of both signs: the sums of maxima stay far below the 2^53 units that make fp64 sums exact."""
    from deltapq_amd import synth
    worst = 0
    for seed in (1, 2, 3):
        _, _, e, _ = R.ip_tables(synth.make_codebook(M, K, Ds, seed), signed_queries(12, M * Ds, seed + 2))
        assert_exact(e, "M=%d K=%d Ds=%d seed=%d" % (M, K, Ds, seed))
        for table in e:
            units, _, g = ne.table_units([[ne.from_f32(v) for v in row] for row in table])
            worst = max(worst, int(units.max(axis=1).sum()))
    print("largest sum of maxima: 2^%.1f units" % np.log2(max(worst, 1)))
    assert worst < 2 ** 53


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M,K,Ds", SHAPES, ids=str)
def test_ip_tables_bit_for_bit(gpu, M, K, Ds):
    import torch
    from deltapq_amd import synth
    cb = synth.make_codebook(M, K, Ds, seed=1)
    tree = ne.plain_tree(65, M, K, seed=2)
    payload, _ = synth.encode_dtc(tree)
    with gpu.DeltaPQIndex.open_memory(payload, 65, M, K) as idx:
        idx.set_codebook(cb)
        for nq in (1, 7, 8, 9, 65):
            qs = signed_queries(nq, M * Ds, seed=3 + nq)
            _, _, e, B = R.ip_tables(cb, qs)
            what = "M=%d K=%d Ds=%d nq=%d" % (M, K, Ds, nq)
            tabs, bias = idx.ip_tables(qs)
            assert tabs.shape == (nq, M, K) and np.array_equal(bits(tabs), bits(e)), what + ": tables (host form)"
            assert np.array_equal(bits(bias), bits(B)), what + ": bias (host form)"
            t_tabs, t_bias = idx.ip_tables_torch(torch.from_numpy(qs).cuda())
            torch.cuda.synchronize()
            assert np.array_equal(bits(t_tabs.cpu().numpy()), bits(e)), what + ": tables (device form)"
            assert np.array_equal(bits(t_bias.cpu().numpy()), bits(B)), what + ": bias (device form)"


# ---- 2. the search ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,nq,ks,opts", [(ne.N_SCAN, 33, (10, 1000), {}), (ne.N_BOOT, 65, (10,), dict(bootstrap=1)),
                                          (ne.N_BOOT, 1, (10,), dict(bootstrap=1, flags=64))],
                         ids=["n4097", "n17001_bootstrap", "n17001_strand1"])
def test_query_batch_ip(gpu, n, nq, ks, opts):
    import torch
    inp = inputs(8, 256, 16, n, nq, seed=1)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], n, 8, 256, **opts) as idx:
        idx.set_codebook(inp["cb"])
        for k in ks:
            what = "n=%d nq=%d top-%d" % (n, nq, k)
            want = expected(inp, k)
            check(idx.query_batch_ip(inp["qs"], k), want, inp["B"], what)
            gaps = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            bias = torch.empty((nq,), dtype=torch.float32, device="cuda")
            ids, scores = idx.query_batch_ip_torch(torch.from_numpy(inp["qs"]).cuda(), k, out_gaps=gaps, out_bias=bias)
            check((ids.cpu().numpy(), scores.cpu().numpy(), gaps.cpu().numpy(), bias.cpu().numpy()), want, inp["B"],
                  what + " (device form)")
            ids2, scores2 = idx.query_batch_ip_torch(torch.from_numpy(inp["qs"]).cuda(), k)     # gaps and bias kept by the handle
            assert np.array_equal(ids2.cpu().numpy(), want[0]) and np.array_equal(bits(scores2.cpu().numpy()), bits(want[2]))


@pytest.mark.gpu
def test_query_batch_ip_m16(gpu):
    inp = inputs(16, 256, 8, ne.N_SCAN, 33, seed=2)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], ne.N_SCAN, 16, 256) as idx:
        idx.set_codebook(inp["cb"])
        check(idx.query_batch_ip(inp["qs"], 10), expected(inp, 10), inp["B"], "M=16")


@pytest.mark.gpu
def test_query_batch_ip_plain_handle(gpu):
    """A dpq_open_plain_* handle accumulates the gap in fp32, m ascending."""
    inp = inputs(8, 256, 16, ne.N_SCAN, 33, seed=1)
    with gpu.DeltaPQIndex.open_plain(inp["codes"], K=256) as idx:
        idx.set_codebook(inp["cb"])
        check(idx.query_batch_ip(inp["qs"], 10), expected(inp, 10, plain=True), inp["B"], "plain handle")


@pytest.mark.gpu
def test_query_batch_ip_two_shards_merge_gaps_then_score(gpu):
    inp = inputs(8, 256, 16, ne.N_SCAN, 33, seed=1)
    k = 10
    parts = []
    for rank in range(2):
        with gpu.DeltaPQIndex.open_memory(inp["payload"], ne.N_SCAN, 8, 256, shard_rank=rank, shard_count=2) as idx:
            idx.set_codebook(inp["cb"])
            info = idx.info()
            got = idx.query_batch_ip(inp["qs"], k)
            check(got, expected(inp, k, lo=info["node_lo"], hi=info["node_hi"]), inp["B"], "rank %d" % rank)
            parts.append(got)
    assert np.array_equal(bits(parts[0][3]), bits(parts[1][3]))                 # the bias does not depend on the shard
    ids, gaps = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[2] for p in parts]))
    want = expected(inp, k)
    check((ids, gpu.ip_scores(parts[0][3], gaps, ids), gaps, parts[0][3]), want, inp["B"], "merged")


@pytest.mark.gpu
def test_query_batch_ip_filtered_pads_with_minus_inf(gpu):
    inp = inputs(8, 256, 16, ne.N_SCAN, 33, seed=1)
    mask = np.zeros(ne.N_SCAN, dtype=bool)
    mask[[3, 77, 1500, 2048, 4096]] = True                                       # fewer ids than top_k
    half = ne.half_mask(ne.N_SCAN, 99)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], ne.N_SCAN, 8, 256) as idx:
        idx.set_codebook(inp["cb"])
        with gpu.IdFilter.from_mask(idx, mask) as f:
            got = idx.query_batch_ip(inp["qs"], 10, id_filter=f)
        check(got, expected(inp, 10, mask), inp["B"], "a few ids")
        assert np.all(got[0][:, 5:] == -1) and np.all(got[0][:, :5] >= 0)
        assert np.all(np.isposinf(got[2][:, 5:])) and np.all(np.isneginf(got[1][:, 5:]))
        with gpu.IdFilter.from_mask(idx, half) as f:
            check(idx.query_batch_ip(inp["qs"], 10, id_filter=f), expected(inp, 10, half), inp["B"], "half mask")


# ---- 3. sanity against plain arithmetic ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M,K,Ds", [(8, 256, 16), (16, 256, 8)], ids=str)
def test_scores_are_the_adc_inner_product(gpu, M, K, Ds):
    """For every reported row, with c_m the code get_codes returns for its id and S = sum_m float64-dot(q_m, c[m][c_m]):
    |s - S| <= (3 M + 4) * 2^-24 * sum_m (|top_m| + |p[m][c_m]|).

    The count, with W = sum_m (|top_m| + |p[m][c_m]|) and u = 2^-24 (one fp32 rounding of x costs at most u |x|):
      per sub-space  p[m][c_m] = float(fp64 dot)   1 rounding  (of |p|          <= W)
                     top_m, a p as well            1 rounding  (of |top_m|      <= W)
                     e = top_m - p                 1 rounding  (of |e| <= |top_m| + |p| <= W)        -> 3 M
      once           g = float(fp64 sum of the e)  1 rounding  (of g <= W; the sum itself is exact)
                     B = float(fp64 sum of top)    1 rounding  (of |B| <= W)
                     (double)B - (double)g         1 rounding in fp64, counted as a whole u W
                     s = float(of that)            1 rounding                                        -> 4
    Each is charged u W although most round something far smaller (the three per-sub-space ones together cost at most
    2 u W over ALL m, and |s| <= 2 W is covered by that slack), so (3 M + 4) u W holds with room: the largest ratio is
    printed.  The fp64 steps inside the dot products are 2^-29 of this.  A wrong sub-space, sign or bias misses the bound
    by orders of magnitude."""
    inp = inputs(M, K, Ds, ne.N_SCAN, 33, seed=2 if M == 16 else 1)
    cb64, q64 = inp["cb"].astype(np.float64), inp["qs"].astype(np.float64).reshape(-1, M, Ds)
    mm = np.arange(M)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], ne.N_SCAN, M, K) as idx:
        idx.set_codebook(inp["cb"])
        ids, scores, _, _ = idx.query_batch_ip(inp["qs"], 100)
        codes = idx.get_codes(ids.reshape(-1)).reshape(ids.shape + (M,))
    assert np.all(ids >= 0)
    worst = 0.0
    for q in range(len(ids)):
        c = cb64[mm[None, :], codes[q]]                                        # [k][M][Ds]
        S = (c * q64[q][None, :, :]).sum(axis=(1, 2))
        W = (np.abs(inp["top"][q].astype(np.float64))[None, :] + np.abs(inp["p"][q][mm[None, :], codes[q]].astype(np.float64))).sum(axis=1)
        bound = (3 * M + 4) * 2.0 ** -24 * W
        err = np.abs(scores[q].astype(np.float64) - S)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), "query %d: |s - S| = %g above the bound %g" % (q, (err - bound).max() + bound.max(), bound.max())
    print("largest |s - S| / bound: %.3f" % worst)
