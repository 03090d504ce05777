"""Range search (dpq_range_search): every code with distance strictly below a per-query radius, against the oracle's
distances of every code.  A range result is a set ordered by (distance, id), so ids and distance bits are compared
exactly.  The CPU tests cover the binding, argument checks and merge_range_host."""
import ctypes

import numpy as np
import pytest

from conftest import make_case


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_range_symbols_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    names = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("dpq_range_search", "dpq_range_result_get", "dpq_range_result_free"):
        assert name in names
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_range_null_arguments(lib):
    out = ctypes.c_void_p(1)
    q = np.zeros((1, 128), dtype=np.float32)
    r = np.ones(1, dtype=np.float32)
    qp, rp = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(r.ctypes.data)
    assert lib.dpq_range_search(None, qp, 1, rp, ctypes.byref(out)) == -1
    assert out.value is None                       # *out is cleared whenever it can be
    assert lib.dpq_range_search(None, qp, 1, rp, None) == -1
    n = ctypes.c_int32()
    pl, pi, pd = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.dpq_range_result_get(None, ctypes.byref(n), ctypes.byref(pl), ctypes.byref(pi), ctypes.byref(pd)) == -1
    lib.dpq_range_result_free(None)


def _keyed(lims, ids, dists):
    return [(ids[lims[q]:lims[q + 1]].tolist(), dists[lims[q]:lims[q + 1]].view(np.uint32).tolist())
            for q in range(len(lims) - 1)]


def test_merge_range_host_hand_built():
    from deltapq_amd.dist import merge_range_host
    f = np.float32
    # query 0: a tie at 1.0 across the parts (ids 7 and 3), query 1: only part B, query 2: nothing anywhere
    a = (np.array([0, 2, 2, 2]), np.array([7, 9], np.int32), np.array([1.0, 2.5], f))
    b = (np.array([0, 2, 4, 4]), np.array([3, 11, 4, 5], np.int32), np.array([1.0, 3.0, 0.5, 0.5], f))
    lims, ids, dists = merge_range_host([a, b])
    assert lims.dtype == np.int64 and ids.dtype == np.int32 and dists.dtype == np.float32
    assert lims.tolist() == [0, 4, 6, 6]
    assert ids.tolist() == [3, 7, 9, 11, 4, 5]
    assert dists.tolist() == [1.0, 1.0, 2.5, 3.0, 0.5, 0.5]
    # one part alone comes back as it was; no queries at all
    assert _keyed(*merge_range_host([b])) == _keyed(*b)
    l0, i0, d0 = merge_range_host([(np.array([0]), np.array([], np.int32), np.array([], f))] * 2)
    assert l0.tolist() == [0] and len(i0) == 0 and len(d0) == 0
    # every part empty for every one of three queries
    nothing = (np.array([0, 0, 0, 0]), np.array([], np.int32), np.array([], f))
    l3, i3, d3 = merge_range_host([nothing, nothing, nothing])
    assert l3.tolist() == [0, 0, 0, 0] and l3.dtype == np.int64 and len(i3) == 0 and len(d3) == 0
    assert i3.dtype == np.int32 and d3.dtype == np.float32
    assert _keyed(*merge_range_host([nothing, b, nothing])) == _keyed(*b)
    # id / distance arrays longer than lims[-1] (a buffer with room to spare): the tail is not part of the answer
    a_long = (a[0], np.array([7, 9, 1, 0], np.int32), np.array([1.0, 2.5, 0.0, 0.25], f))
    b_long = (b[0], np.concatenate((b[1], np.array([2], np.int32))), np.concatenate((b[2], np.array([0.125], f))))
    assert _keyed(*merge_range_host([a_long, b_long])) == _keyed(lims, ids, dists)
    # parts that answer different numbers of queries, and no parts at all
    with pytest.raises(ValueError):
        merge_range_host([a, (np.array([0, 2, 4]), b[1], b[2])])
    with pytest.raises(ValueError):
        merge_range_host([(np.array([0, 2, 4]), b[1], b[2]), a])
    with pytest.raises(ValueError):
        merge_range_host([])


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
    return ids.astype(np.int32)


def expected_list(all_d, r, n_total, id_rule=True):
    pos = np.flatnonzero(all_d < np.float32(r))
    order = np.lexsort((pos, all_d[pos].view(np.uint32)))
    pos = pos[order]
    return (report_ids(pos, n_total) if id_rule else pos.astype(np.int32)), all_d[pos]


def radius_menu(all_d, i):
    """Per-query radius kinds: 0, below every distance, exactly the 10th (excluded), just above it, median, +inf."""
    s = np.sort(all_d)
    tenth = s[min(9, len(s) - 1)]
    kind = i % 6
    if kind == 0:
        return np.float32(0.0)
    if kind == 1:
        return np.float32(s[0] * np.float32(0.5)) if s[0] > 0 else np.float32(0.0)
    if kind == 2:
        return tenth
    if kind == 3:
        return np.nextafter(tenth, np.float32(np.inf))
    if kind == 4:
        return s[len(s) // 2]
    return np.float32(np.inf)


def assert_range_equal(got, want, what=""):
    lims, ids, dists = got
    assert len(lims) == len(want) + 1 and lims[0] == 0, what
    for q, (wi, wd) in enumerate(want):
        gi, gd = ids[lims[q]:lims[q + 1]], dists[lims[q]:lims[q + 1]]
        assert len(gi) == len(wi), "%s query %d: %d results, expected %d" % (what, q, len(gi), len(wi))
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), "%s query %d: distances differ" % (what, q)
        assert np.array_equal(gi, wi), "%s query %d: ids differ" % (what, q)


def oracle_all(oracle, payload, n, cb, qs):
    return [oracle.scan_lut(payload, n, oracle.build_lut(cb, q), 1, want_all=True)[2] for q in qs]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 9999, 100000, 300001])
def test_range_parity_with_oracle(gpu, oracle, codebook, n):
    from deltapq_amd import synth
    _, payload, _ = make_case(n, seed=n + 31)
    qs = synth.make_queries(12, 128, seed=n + 32)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    radii = np.array([radius_menu(alld[i], i) for i in range(len(qs))], dtype=np.float32)
    want = [expected_list(alld[i], radii[i], n) for i in range(len(qs))]
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        got = idx.range_search(qs, radii)
    assert_range_equal(got, want, "n=%d" % n)
    lims = got[0]
    assert lims[1] == 0 and lims[6] - lims[5] == n           # radius 0: nothing; +inf: every code


@pytest.fixture(scope="module")
def plan_case(oracle, codebook):
    from deltapq_amd import synth
    n = 20000
    _, payload, _ = make_case(n, seed=5)
    qs = synth.make_queries(2049, 128, seed=6)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    radii = np.array([radius_menu(alld[i], i) for i in range(len(qs))], dtype=np.float32)
    want = [expected_list(alld[i], radii[i], n) for i in range(len(qs))]
    return n, payload, qs, radii, want


@pytest.mark.gpu
@pytest.mark.parametrize("batch_decode", [-1, 1, 2])
@pytest.mark.parametrize("bootstrap", [1, -1])
def test_range_every_batched_plan(gpu, codebook, plan_case, batch_decode, bootstrap):
    n, payload, qs, radii, want = plan_case
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, batch_decode=batch_decode, bootstrap=bootstrap) as idx:
        idx.set_codebook(codebook)
        for nq in (1, 63, 65, 200, 2049):               # 2049: two sub-batches
            got = idx.range_search(qs[:nq], radii[:nq])
            assert_range_equal(got, want[:nq], "batch_decode=%d bootstrap=%d nq=%d" % (batch_decode, bootstrap, nq))


@pytest.mark.gpu
def test_range_forced_overflow_reruns_exactly(gpu, oracle, codebook):
    from deltapq_amd import synth
    n = 100000
    _, payload, _ = make_case(n, seed=41)
    qs = synth.make_queries(70, 128, seed=42)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    radii = np.array([np.sort(d)[2000 + 37 * i] for i, d in enumerate(alld)], dtype=np.float32)   # thousands per query
    want = [expected_list(alld[i], radii[i], n) for i in range(len(qs))]
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, cand_capacity=256) as idx:
        idx.set_codebook(codebook)
        idx.profile_enable(True)
        got = idx.range_search(qs, radii)
        prof = idx.profile_read()
    assert_range_equal(got, want, "cand_capacity=256")
    assert prof["overflow_reruns"] > 0 and prof["queries"] == len(qs)


@pytest.mark.gpu
def test_range_rerun_lays_out_regions_for_live_queries_only(gpu, oracle, codebook, monkeypatch):
    """A rerun of overflowed +inf lists takes about N keys per query, not a whole query group's worth (64 x N)."""
    from deltapq_amd import synth
    n = 300001
    _, payload, _ = make_case(n, seed=45)
    qs = synth.make_queries(3, 128, seed=46)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, cand_capacity=256) as idx:
        idx.set_codebook(codebook)
        idx.profile_enable(True)
        keys = ctypes.c_int64()
        for nq in (1, 3):
            got = idx.range_search(qs[:nq], np.inf)
            assert_range_equal(got, [expected_list(d, np.inf, n) for d in alld[:nq]], "+inf nq=%d" % nq)
            monkeypatch.setenv("DPQ_DEV", "1")
            assert idx._lib.dpq_debug_range_keys(idx._h, ctypes.byref(keys)) == 0
            monkeypatch.delenv("DPQ_DEV")
            assert n * nq <= keys.value <= 2 * n * nq, (nq, keys.value)
        assert idx.profile_read()["overflow_reruns"] == 4


@pytest.mark.gpu
def test_range_agrees_with_topk(gpu, codebook):
    from oracle.dtc_oracle import tie_aware_equal
    from deltapq_amd import synth
    n, k = 100000, 100
    _, payload, _ = make_case(n, seed=51)
    qs = synth.make_queries(80, 128, seed=52)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        ids, dists = idx.query_batch(qs, k)
        radii = np.nextafter(dists[:, -1], np.float32(np.inf))
        lims, rids, rd = idx.range_search(qs, radii)
    for q in range(len(qs)):
        gi, gd = rids[lims[q]:lims[q + 1]], rd[lims[q]:lims[q + 1]]
        assert len(gi) >= k and np.all(gd <= dists[q, -1])
        ok, msg = tie_aware_equal(gi[:k], gd[:k], ids[q], dists[q])
        assert ok, "query %d: %s" % (q, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 100001])
def test_range_m16(gpu, oracle, n):
    from deltapq_amd import synth
    cb = synth.make_codebook(16, 256, 8, seed=3)
    tree = synth.synth_tree(n, 16, seed=n + 1, mean_diffs=5.0)
    payload, _ = synth.encode_dtc(tree)
    qs = synth.make_queries(40, 128, seed=n + 2)
    alld = oracle_all(oracle, payload, n, cb, qs)
    radii = np.array([radius_menu(alld[i], i) for i in range(len(qs))], dtype=np.float32)
    want = [expected_list(alld[i], radii[i], n) for i in range(len(qs))]
    with gpu.DeltaPQIndex.open_memory(payload, n, 16, 256) as idx:
        idx.set_codebook(cb)
        got = idx.range_search(qs, radii)
    assert_range_equal(got, want, "M=16 n=%d" % n)


def plain_dists(lut, codes):
    d = np.zeros(len(codes), dtype=np.float32)
    for m in range(codes.shape[1]):
        d = (d + lut[m, codes[:, m]]).astype(np.float32)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("n,M", [(20000, 8), (50000, 16)])
def test_range_plain_index_fp32_rule(gpu, oracle, n, M):
    from deltapq_amd import synth
    rng = np.random.default_rng(n)
    protos = rng.integers(0, 256, size=(n // 20, M), dtype=np.uint8)
    codes = protos[rng.integers(0, len(protos), size=n)].copy()        # duplicates -> ties
    codes[np.arange(n), rng.integers(0, M, size=n)] = rng.integers(0, 256, size=n)
    cb = synth.make_codebook(M, 256, 128 // M, seed=1)
    qs = synth.make_queries(30, 128, seed=2)
    alld = [plain_dists(oracle.build_lut(cb, q), codes) for q in qs]
    radii = np.array([radius_menu(alld[i], i) for i in range(len(qs))], dtype=np.float32)
    want = [expected_list(alld[i], radii[i], n, id_rule=False) for i in range(len(qs))]
    with gpu.DeltaPQIndex.open_plain(codes) as idx:
        idx.set_codebook(cb)
        got = idx.range_search(qs, radii)
    assert_range_equal(got, want, "plain M=%d" % M)


@pytest.mark.gpu
def test_range_shards_merge_to_the_whole(gpu, codebook):
    from deltapq_amd import synth
    from deltapq_amd.dist import merge_range_host
    n = 100000
    _, payload, _ = make_case(n, seed=61)
    qs = synth.make_queries(40, 128, seed=62)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        _, d = idx.query_batch(qs, 300)
        radii = d[:, -1]
        whole = idx.range_search(qs, radii)
    parts = []
    for r in range(2):
        with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, shard_rank=r, shard_count=2) as idx:
            idx.set_codebook(codebook)
            parts.append(idx.range_search(qs, radii))
    assert all(p[0][-1] > 0 for p in parts)
    merged = merge_range_host(parts)
    for a, b in zip(merged, whole):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.gpu
def test_range_full_size_1m(gpu, oracle):
    from deltapq_amd import synth
    n, nq, k = 1_000_000, 1000, 100
    cb = synth.make_codebook(8, 256, 16, seed=0)
    tree = synth.synth_tree(n, 8, seed=71)
    payload, _ = synth.encode_dtc(tree)
    del tree
    qs = synth.make_queries(nq, 128, seed=72)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(cb)
        ids, dists = idx.query_batch(qs, k)
        radii = np.nextafter(dists[:, -1], np.float32(np.inf))
        lims, rids, rd = idx.range_search(qs, radii)
    counts = np.diff(lims)
    assert np.all(counts >= k)
    for q in range(nq):
        gi, gd = rids[lims[q]:lims[q + 1]], rd[lims[q]:lims[q + 1]]
        assert np.array_equal(gi[:k], ids[q]) and np.array_equal(gd[:k].view(np.uint32), dists[q].view(np.uint32)), q
        assert np.all(gd <= dists[q, -1])
    for q in (0, 499, 999):
        alld = oracle.scan_lut(payload, n, oracle.build_lut(cb, qs[q]), 1, want_all=True)[2]
        wi, wd = expected_list(alld, radii[q], n)
        assert np.array_equal(rids[lims[q]:lims[q + 1]], wi) and np.array_equal(rd[lims[q]:lims[q + 1]], wd), q


@pytest.mark.gpu
def test_range_infinite_radius_returns_every_code_in_order(gpu, oracle, codebook):
    from deltapq_amd import synth
    n = 100000
    _, payload, _ = make_case(n, seed=81)
    qs = synth.make_queries(8, 128, seed=82)
    alld = oracle_all(oracle, payload, n, codebook, qs)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        got = idx.range_search(qs, np.inf)
    assert got[0].tolist() == [n * i for i in range(len(qs) + 1)]
    assert_range_equal(got, [expected_list(d, np.inf, n) for d in alld], "+inf")


@pytest.mark.gpu
def test_range_does_not_disturb_topk(gpu, codebook):
    import torch
    from deltapq_amd import synth
    n, k = 100000, 100
    _, payload, _ = make_case(n, seed=91)
    qs = synth.make_queries(300, 128, seed=92)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        before = idx.query_batch(qs, k)
        ref = idx.range_search(qs[:50], before[1][:50, 20])
        after = idx.query_batch(qs, k)
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # a range search while asynchronous batches are pending: it finishes them first, both answers stay right
        qd = [torch.from_numpy(qs[i * 100:(i + 1) * 100]).cuda() for i in range(3)]
        outs = [idx.query_batch_torch(q, k, wait=False) for q in qd]
        got = idx.range_search(qs[:50], before[1][:50, 20])
        idx.finish()
        for a, b in zip(got, ref):
            assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
        for i, (oi, od) in enumerate(outs):
            assert np.array_equal(oi.cpu().numpy(), before[0][i * 100:(i + 1) * 100])
            assert np.array_equal(od.cpu().numpy().view(np.uint32), before[1][i * 100:(i + 1) * 100].view(np.uint32))


@pytest.mark.gpu
def test_range_errors(gpu, codebook):
    from deltapq_amd import api, synth
    n = 1000
    _, payload, _ = make_case(n, seed=3)
    qs = synth.make_queries(4, 128, seed=4)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        with pytest.raises(api.DpqError) as e:
            idx.range_search(qs, 1.0)                       # no codebook yet
        assert e.value.status == -7
        idx.set_codebook(codebook)
        with pytest.raises(api.DpqError) as e:
            idx.range_search(qs, np.array([1.0, np.nan, 2.0, 3.0], dtype=np.float32))
        assert e.value.status == -1
        lims, ids, dists = idx.range_search(np.zeros((0, 128), dtype=np.float32), 1.0)
        assert lims.tolist() == [0] and len(ids) == 0 and len(dists) == 0
