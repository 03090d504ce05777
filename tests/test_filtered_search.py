"""Filtered top-k search (dpq_query_batch_filtered): the k nearest codes among those an id bitmap allows, against the
oracle's distances of every code masked by the filter, ordered by (distance bits, reported id), cut to k and padded.
Ids and distance bits are compared exactly.  The CPU tests cover the binding, argument checks and IdFilter's packing."""
import ctypes

import numpy as np
import pytest

from conftest import make_case


# ---- CPU ------------------------------------------------------------------------------------------------------------

FILTER_SYMBOLS = ("dpq_filter_create", "dpq_filter_free", "dpq_filter_count", "dpq_query_batch_filtered",
                  "dpq_query_batch_device_filtered")


def test_filter_symbols_declared_exported_and_bound(lib):
    import os
    from deltapq_amd import _lib
    names = {name for name, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "deltapq_amd.h")).read()
    for name in FILTER_SYMBOLS:
        assert name in names
        assert name + "(" in header
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_filter_null_arguments(lib):
    out = ctypes.c_void_p(1)
    words = np.ones(4, dtype=np.uint32)
    wp = ctypes.c_void_p(words.ctypes.data)
    assert lib.dpq_filter_create(None, wp, 100, ctypes.byref(out)) == -1
    assert out.value is None                       # *out is cleared whenever it can be
    assert lib.dpq_filter_create(None, wp, 100, None) == -1
    assert lib.dpq_filter_create(None, wp, -1, ctypes.byref(out)) == -1
    n = ctypes.c_int64()
    assert lib.dpq_filter_count(None, ctypes.byref(n)) == -1
    q = np.zeros((1, 128), dtype=np.float32)
    ids = np.zeros(1, dtype=np.int32)
    d = np.zeros(1, dtype=np.float32)
    qp, ip, dp = (ctypes.c_void_p(a.ctypes.data) for a in (q, ids, d))
    assert lib.dpq_query_batch_filtered(None, None, qp, 1, 1, ip, dp) == -1
    assert lib.dpq_query_batch_device_filtered(None, None, qp, 1, 1, ip, dp, None) == -1
    lib.dpq_filter_free(None)


def test_id_filter_packing_little_endian():
    from deltapq_amd.api import IdFilter
    words, n = IdFilter.pack_ids([0, 5, 31, 32, 70], 71)
    assert n == 71 and words.dtype == np.uint32
    assert words.tolist() == [(1 << 0) | (1 << 5) | (1 << 31), 1 << 0, 1 << 6]
    mask = IdFilter.unpack(words, n)
    assert mask.dtype == bool and len(mask) == 71 and np.flatnonzero(mask).tolist() == [0, 5, 31, 32, 70]
    rng = np.random.default_rng(1)
    for size in (0, 1, 31, 32, 33, 64, 1000, 4099):
        m = rng.random(size) < 0.3
        w, nb = IdFilter.pack_mask(m)
        assert nb == size and len(w) == (size + 31) // 32
        assert np.array_equal(IdFilter.unpack(w, nb), m)
        for i in np.flatnonzero(m):                 # bit i is bit (i & 31) of word i >> 5
            assert (int(w[i >> 5]) >> (i & 31)) & 1
        w2, nb2 = IdFilter.pack_ids(np.flatnonzero(m), size)
        assert nb2 == size and np.array_equal(w2, w)
    assert IdFilter.pack_ids([3, 9])[1] == 10       # n_bits defaults to max(id) + 1
    with pytest.raises(ValueError):
        IdFilter.pack_ids([5], 5)


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def report_ids(pos, n_total):
    """The even-N rule: the last DFS node of an even-N index is reported as N."""
    ids = pos.astype(np.int64)
    if n_total % 2 == 0:
        ids[ids == n_total - 1] = n_total
    return ids


def expected_topk(all_d, mask, k, n_total, id_rule=True):
    """The filtered answer: codes whose reported id is allowed by `mask`, by (distance bits, id), cut to k, padded."""
    pos = np.arange(len(all_d), dtype=np.int64)
    rep = report_ids(pos, n_total) if id_rule else pos
    ok = rep < len(mask)
    ok[ok] = mask[rep[ok]]
    p = pos[ok]
    keys = (all_d[p].view(np.uint32).astype(np.uint64) << np.uint64(32)) | p.astype(np.uint64)
    if len(keys) > k:
        keys = np.partition(keys, k - 1)[:k]
    keys = np.sort(keys)
    sel = (keys & np.uint64(0xffffffff)).astype(np.int64)
    ids = np.full(k, -1, dtype=np.int32)
    d = np.full(k, np.inf, dtype=np.float32)
    ids[:len(sel)] = rep[sel]
    d[:len(sel)] = all_d[sel]
    return ids, d


def assert_rows_equal(got, want, what=""):
    gi, gd = got
    for q, (wi, wd) in enumerate(want):
        assert np.array_equal(gd[q].view(np.uint32), wd.view(np.uint32)), "%s query %d: distances differ\n got %s\n want %s" % (
            what, q, gd[q][:8], wd[:8])
        assert np.array_equal(gi[q], wi), "%s query %d: ids differ\n got %s\n want %s" % (what, q, gi[q][:8], wi[:8])


def assert_same(a, b, what=""):
    assert np.array_equal(a[0], b[0]), what + ": ids differ"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), what + ": distances differ"


def oracle_all(oracle, payload, n, cb, qs):
    return [oracle.scan_lut(payload, n, oracle.build_lut(cb, q), 1, want_all=True)[2] for q in qs]


def random_mask(n_bits, frac, seed):
    return np.random.default_rng(seed).random(n_bits) < frac


@pytest.fixture(scope="module")
def boot_case(oracle, codebook):
    """100 000 codes (a bootstrap shard), 1000 queries and the oracle's distances of the first 120."""
    from deltapq_amd import synth
    n = 100000
    _, payload, _ = make_case(n, seed=11)
    qs = synth.make_queries(1000, 128, seed=12)
    return n, payload, qs, oracle_all(oracle, payload, n, codebook, qs[:120])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 100000])
@pytest.mark.parametrize("batch_decode", [-1, 1, 2])
def test_all_ones_filter_equals_unfiltered(gpu, codebook, boot_case, n, batch_decode):
    """Level 0 (20 000 codes) and bootstrap (100 000) shards; decode inside the scan, one plain-code tile, tiles of two
    segments.  nq = 1 and 3 are stream-pass batches unfiltered and filter-scan batches filtered."""
    from deltapq_amd import synth
    if n == boot_case[0]:
        payload, qs = boot_case[1], boot_case[2]
    else:
        _, payload, _ = make_case(n, seed=13)
        qs = synth.make_queries(1000, 128, seed=14)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, batch_decode=batch_decode) as idx:
        idx.set_codebook(codebook)
        assert (idx.info()["bootstrap_bytes"] > 0) == (n >= 65536)
        with gpu.IdFilter.from_mask(idx, np.ones(n + 1, dtype=bool)) as f:   # (bit N: the last node of an even N)
            assert f.n_allowed == n
            for k in (1, 100, 1000, 2048):
                for nq in (1, 3, 64, 200, 1000):
                    assert_same(idx.query_batch_filtered(qs[:nq], k, f), idx.query_batch(qs[:nq], k),
                                "n=%d batch_decode=%d k=%d nq=%d" % (n, batch_decode, k, nq))


def _selectivity_check(gpu, idx, qs, alld, n, frac, seed, k=100, id_rule=True, what=""):
    mask = random_mask(n + 1, frac, seed)
    with gpu.IdFilter.from_mask(idx, mask) as f:
        got = idx.query_batch_filtered(qs, k, f)
    assert_rows_equal(got, [expected_topk(d, mask, k, n, id_rule) for d in alld], "%s frac=%g" % (what, frac))


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.5, 0.1, 0.01, 0.001])
def test_random_filters_dtc_m8(gpu, oracle, codebook, boot_case, frac):
    n, payload, qs, alld = boot_case
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        for nq in (2, 120):                             # one query group; two
            _selectivity_check(gpu, idx, qs[:nq], alld[:nq], n, frac, seed=int(frac * 1e4) + nq, what="M=8 nq=%d" % nq)
    _, p2, _ = make_case(30000, seed=15)                 # level 0 + filter levels
    from deltapq_amd import synth
    q2 = synth.make_queries(70, 128, seed=16)
    a2 = oracle_all(oracle, p2, 30000, codebook, q2)
    with gpu.DeltaPQIndex.open_memory(p2, 30000, 8, 256) as idx:
        idx.set_codebook(codebook)
        _selectivity_check(gpu, idx, q2, a2, 30000, frac, seed=17, k=50, what="M=8 level 0")


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.5, 0.1, 0.01, 0.001])
def test_random_filters_dtc_m16(gpu, oracle, frac):
    from deltapq_amd import synth
    n = 100001
    cb = synth.make_codebook(16, 256, 8, seed=3)
    tree = synth.synth_tree(n, 16, seed=n + 1, mean_diffs=5.0)
    payload, _ = synth.encode_dtc(tree)
    qs = synth.make_queries(70, 128, seed=n + 2)
    alld = oracle_all(oracle, payload, n, cb, qs)
    with gpu.DeltaPQIndex.open_memory(payload, n, 16, 256) as idx:
        idx.set_codebook(cb)
        _selectivity_check(gpu, idx, qs, alld, n, frac, seed=21, what="M=16")


def plain_dists(lut, codes):
    d = np.zeros(len(codes), dtype=np.float32)
    for m in range(codes.shape[1]):
        d = (d + lut[m, codes[:, m]]).astype(np.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.5, 0.1, 0.01, 0.001])
def test_random_filters_plain_fp32_rule(gpu, oracle, frac):
    from deltapq_amd import synth
    n, M = 100000, 8
    rng = np.random.default_rng(n)
    protos = rng.integers(0, 256, size=(n // 20, M), dtype=np.uint8)
    codes = protos[rng.integers(0, len(protos), size=n)].copy()        # duplicates -> ties
    codes[np.arange(n), rng.integers(0, M, size=n)] = rng.integers(0, 256, size=n)
    cb = synth.make_codebook(M, 256, 128 // M, seed=1)
    qs = synth.make_queries(70, 128, seed=2)
    alld = [plain_dists(oracle.build_lut(cb, q), codes) for q in qs]
    with gpu.DeltaPQIndex.open_plain(codes) as idx:                    # (even n: no id rule on a plain index)
        idx.set_codebook(cb)
        _selectivity_check(gpu, idx, qs, alld, n, frac, seed=23, id_rule=False, what="plain")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
def test_adversarial_filter_removes_every_querys_nearest(gpu, oracle, codebook, k):
    """The filter removes the union of every query's unfiltered top-500: a bootstrap or an in-scan tightening that counted
    a removed node would cut below the true k-th key and lose results.  600 queries: tightening and bootstrap both live."""
    from deltapq_amd import synth
    n, nq = 200000, 600
    _, payload, _ = make_case(n, seed=31)
    qs = synth.make_queries(nq, 128, seed=32)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        top, _ = idx.query_batch(qs, 500)
        mask = np.ones(n + 1, dtype=bool)                # (ids up to N: the even-N rule)
        mask[top.ravel()] = False
        assert 0 < mask.sum() < n
        with gpu.IdFilter.from_mask(idx, mask) as f:
            idx.profile_enable(True)
            got = idx.query_batch_filtered(qs, k, f)
            prof = idx.profile_read()
    # the same call without the in-scan tightening: its thresholds stay at the bootstrap's, so at top-100 it takes more
    # candidates -- the tightening was live above (and its cuts, counted from allowed nodes only, lost nothing).  (At
    # top-10 the bootstrap's cut is already within a step of the tables' resolution: nothing left to lower.)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, flags=gpu.OPT_NO_TIGHTEN) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            idx.profile_enable(True)
            got_nt = idx.query_batch_filtered(qs, k, f)
            prof_nt = idx.profile_read()
    assert prof["bootstrap_launches"] >= 1 and prof_nt["bootstrap_launches"] >= 1
    if k >= 100:
        assert prof["candidates"] < prof_nt["candidates"], (prof["candidates"], prof_nt["candidates"])
    alld = oracle_all(oracle, payload, n, codebook, qs)
    want = [expected_topk(d, mask, k, n) for d in alld]
    assert_rows_equal(got, want, "adversarial k=%d" % k)
    assert_rows_equal(got_nt, want, "adversarial k=%d, no tightening" % k)
    assert not np.isin(got[0], top).any()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [641, 1000])
@pytest.mark.parametrize("frac", [0.01, 0.05])
def test_bootstrap_round_beyond_65535_nodes(gpu, oracle, k, frac):
    """Every code shares sub-spaces 0 and 1: one multi-index cell holds all 200 000 nodes, so the round that reaches it
    holds more nodes than its 16-bit prefix can address.  A large top_k (cap 12 288) and a filter that allows few of them
    make the filtered bootstrap walk past 65 535 nodes of that round if nothing stops it."""
    from deltapq_amd import synth
    n, M = 200000, 8
    rng = np.random.default_rng(7)
    protos = rng.integers(0, 256, size=(n // 50, M), dtype=np.uint8)
    codes = protos[rng.integers(0, len(protos), size=n)].copy()
    codes[:, 0], codes[:, 1] = 17, 201
    cb = synth.make_codebook(M, 256, 128 // M, seed=8)
    qs = synth.make_queries(40, 128, seed=9)
    alld = [plain_dists(oracle.build_lut(cb, q), codes) for q in qs]
    mask = random_mask(n, frac, 10)
    with gpu.DeltaPQIndex.open_plain(codes, bootstrap=1) as idx:
        idx.set_codebook(cb)
        assert idx.info()["bootstrap_bytes"] > 0
        with gpu.IdFilter.from_mask(idx, mask) as f:
            idx.profile_enable(True)
            got = idx.query_batch_filtered(qs, k, f)
            assert idx.profile_read()["bootstrap_launches"] >= 1
    assert_rows_equal(got, [expected_topk(d, mask, k, n, id_rule=False) for d in alld], "dense cell k=%d frac=%g" % (k, frac))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 100000])
def test_few_or_no_eligible_codes_pad(gpu, oracle, codebook, boot_case, n):
    from deltapq_amd import synth
    if n == boot_case[0]:
        payload, qs, alld = boot_case[1], boot_case[2][:70], boot_case[3][:70]
    else:
        _, payload, _ = make_case(n, seed=41)
        qs = synth.make_queries(70, 128, seed=42)
        alld = oracle_all(oracle, payload, n, codebook, qs)
    allowed = np.random.default_rng(43).choice(n - 1, 37, replace=False)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_ids(idx, allowed, n + 1) as f:
            assert f.n_allowed == 37
            for nq in (1, 70):
                got = idx.query_batch_filtered(qs[:nq], 100, f)
                mask = np.zeros(n + 1, dtype=bool)
                mask[allowed] = True
                assert_rows_equal(got, [expected_topk(d, mask, 100, n) for d in alld[:nq]], "37 allowed nq=%d" % nq)
                assert np.all(got[0][:, 37:] == -1) and np.all(np.isinf(got[1][:, 37:]))
        for words, bits in ((np.zeros(0, dtype=np.uint32), 0), (np.zeros((n + 31) // 32, dtype=np.uint32), n)):
            with gpu.IdFilter(idx, words, bits) as f:
                assert f.n_allowed == 0
                for nq in (1, 70):
                    ids, d = idx.query_batch_filtered(qs[:nq], 50, f)
                    assert np.all(ids == -1) and np.all(np.isinf(d))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 100000])
def test_even_n_rule(gpu, oracle, codebook, boot_case, n):
    """Bit N selects the last node of an even-N index (reported as N); bit N - 1 alone selects nothing."""
    from deltapq_amd import synth
    if n == boot_case[0]:
        payload, qs, alld = boot_case[1], boot_case[2][:70], boot_case[3][:70]
    else:
        _, payload, _ = make_case(n, seed=51)
        qs = synth.make_queries(70, 128, seed=52)
        alld = oracle_all(oracle, payload, n, codebook, qs)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_ids(idx, [n]) as f:
            assert f.n_allowed == 1
            ids, d = idx.query_batch_filtered(qs, 5, f)
            assert np.all(ids[:, 0] == n) and np.all(ids[:, 1:] == -1)
            assert np.array_equal(d[:, 0].view(np.uint32), np.array([a[n - 1] for a in alld], np.float32).view(np.uint32))
        with gpu.IdFilter.from_ids(idx, [n - 1]) as f:
            assert f.n_allowed == 0
            ids, d = idx.query_batch_filtered(qs, 5, f)
            assert np.all(ids == -1) and np.all(np.isinf(d))
        mask = random_mask(n + 1, 0.02, 53)
        mask[n], mask[n - 1] = True, False
        with gpu.IdFilter.from_mask(idx, mask) as f:
            got = idx.query_batch_filtered(qs, 100, f)
        assert_rows_equal(got, [expected_topk(a, mask, 100, n) for a in alld], "even N=%d" % n)


@pytest.mark.gpu
def test_num_codes_prefix_even_rule(gpu, oracle, codebook):
    """num_codes = 20 000 of a 30 000-code payload: N = 20 000 under the same rule (bit N selects node N - 1)."""
    from deltapq_amd import synth
    n, n_scan = 30000, 20000
    tree, payload, _ = make_case(n, seed=61)
    sub = dict(root=tree["root"], depths=tree["depths"][:n_scan], masks=tree["masks"][:n_scan], M=8,
               deltas=tree["deltas"][:int(sum(bin(int(m)).count("1") for m in tree["masks"][1:n_scan]))])
    p2, _ = synth.encode_dtc(sub)
    qs = synth.make_queries(40, 128, seed=62)
    alld = oracle_all(oracle, p2, n_scan, codebook, qs)
    mask = random_mask(n, 0.05, 63)
    mask[n_scan] = True
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, num_codes=n_scan) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            assert f.n_allowed == int(mask[:n_scan - 1].sum()) + 1
            got = idx.query_batch_filtered(qs, 100, f)
    assert_rows_equal(got, [expected_topk(a, mask, 100, n_scan) for a in alld], "num_codes")


@pytest.mark.gpu
def test_dup_heavy_ties(gpu, oracle, codebook):
    from deltapq_amd import synth
    n = 100000
    _, payload, _ = make_case(n, seed=71, dup_heavy=True)
    qs = synth.make_queries(70, 128, seed=72)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        for frac in (0.3, 0.01):
            _selectivity_check(gpu, idx, qs, alld, n, frac, seed=73, what="dup_heavy")


@pytest.mark.gpu
def test_forced_overflow_reruns_exactly(gpu, oracle, codebook):
    """cand_capacity=256 at low selectivity: the bootstrap finds few allowed keys, regions overflow, the rerun is exact."""
    from deltapq_amd import synth
    n = 100000
    _, payload, _ = make_case(n, seed=81)
    qs = synth.make_queries(70, 128, seed=82)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    mask = random_mask(n + 1, 0.005, 83)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, cand_capacity=256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            idx.profile_enable(True)
            got = idx.query_batch_filtered(qs, 100, f)
            prof = idx.profile_read()
    assert prof["overflow_reruns"] > 0
    assert_rows_equal(got, [expected_topk(d, mask, 100, n) for d in alld], "cand_capacity=256")


@pytest.mark.gpu
def test_shards_merge_to_the_whole(gpu, codebook):
    """Two shards of 100 000 nodes: each has a bootstrap, whose multi-index ids start at the shard's base."""
    n, k = 200000, 100
    from deltapq_amd import synth
    _, payload, _ = make_case(n, seed=91)
    qs = synth.make_queries(80, 128, seed=92)
    mask = random_mask(n + 1, 0.1, 93)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            whole = idx.query_batch_filtered(qs, k, f)
    parts = []
    for r in range(2):
        with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, shard_rank=r, shard_count=2) as idx:
            idx.set_codebook(codebook)
            assert idx.info()["bootstrap_bytes"] > 0 and (idx.info()["node_lo"] > 0) == (r == 1)
            with gpu.IdFilter.from_mask(idx, mask) as f:
                assert 0 < f.n_allowed < mask.sum()
                idx.profile_enable(True)
                parts.append(idx.query_batch_filtered(qs, k, f))
                assert idx.profile_read()["bootstrap_launches"] >= 1
    merged = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert_same(merged, whole, "two shards")


@pytest.mark.gpu
def test_device_entry_point_with_torch(gpu, codebook, boot_case):
    import torch
    n, payload, qs, _ = boot_case
    mask = random_mask(n, 0.2, 101)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            for nq in (1, 300):
                want = idx.query_batch_filtered(qs[:nq], 64, f)
                ti, td = idx.query_batch_filtered_torch(torch.from_numpy(qs[:nq]).cuda(), 64, f)
                torch.cuda.synchronize()
                assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "torch nq=%d" % nq)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20000, 100000])
def test_unfiltered_results_unchanged_by_filtered_calls(gpu, codebook, boot_case, n):
    """The plan cache, the level-0 list and both lanes' workspaces give the same unfiltered answers after filtered calls."""
    import torch
    from deltapq_amd import synth
    if n == boot_case[0]:
        payload, qs = boot_case[1], boot_case[2]
    else:
        _, payload, _ = make_case(n, seed=111)
        qs = synth.make_queries(1000, 128, seed=112)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        shapes = ((1, 100), (3, 10), (1000, 100), (200, 1000))
        before = [idx.query_batch(qs[:nq], k) for nq, k in shapes]
        qd = [torch.from_numpy(qs[i * 500:(i + 1) * 500]).cuda() for i in range(2)]
        outs0 = [idx.query_batch_torch(q, 100, wait=False) for q in qd]   # both lanes
        idx.finish()
        with gpu.IdFilter.from_mask(idx, random_mask(n, 0.05, 113)) as f:
            for nq, k in shapes:
                idx.query_batch_filtered(qs[:nq], k, f)
            # a filtered call while asynchronous batches are pending finishes them first
            outs = [idx.query_batch_torch(q, 100, wait=False) for q in qd]
            idx.query_batch_filtered(qs[:64], 100, f)
            idx.finish()
        for (nq, k), b in zip(shapes, before):
            assert_same(idx.query_batch(qs[:nq], k), b, "after filtered calls nq=%d k=%d" % (nq, k))
        for (i0, d0), (i1, d1) in zip(outs0, outs):
            assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
        outs2 = [idx.query_batch_torch(q, 100, wait=False) for q in qd]
        idx.finish()
        for (i0, d0), (i2, d2) in zip(outs0, outs2):
            assert torch.equal(i0, i2) and torch.equal(d0.view(torch.int32), d2.view(torch.int32))


@pytest.mark.gpu
def test_filter_errors(gpu, codebook):
    from deltapq_amd import api, synth
    n = 1000
    _, payload, _ = make_case(n, seed=121)
    qs = synth.make_queries(4, 128, seed=122)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as a, gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as b:
        a.set_codebook(codebook)
        b.set_codebook(codebook)
        fb = gpu.IdFilter.from_mask(b, np.ones(n, dtype=bool))
        with pytest.raises(api.DpqError) as e:
            a.query_batch_filtered(qs, 10, fb)            # made on another handle
        assert e.value.status == -1
        ids, _ = b.query_batch_filtered(qs, 10, fb)
        assert np.all(ids >= 0)
        fb.close()
        with pytest.raises(TypeError):
            a.query_batch_filtered(qs, 10, None)
        out = ctypes.c_void_p()
        q = np.ascontiguousarray(qs)
        i = np.zeros((4, 10), dtype=np.int32)
        d = np.zeros((4, 10), dtype=np.float32)
        assert a._lib.dpq_query_batch_filtered(a._h, None, ctypes.c_void_p(q.ctypes.data), 4, 10,
                                               ctypes.c_void_p(i.ctypes.data), ctypes.c_void_p(d.ctypes.data)) == -1
        assert a._lib.dpq_filter_create(a._h, None, -1, ctypes.byref(out)) == -1 and out.value is None
        with gpu.IdFilter.from_mask(a, np.ones(n, dtype=bool)) as f:
            with pytest.raises(api.DpqError) as e:
                a.query_batch_filtered(qs, 0, f)          # top_k out of range, as for dpq_query_batch
            assert e.value.status == -1
