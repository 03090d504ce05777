"""Candidate search (dpq_candidate_search*, dpq_candidate_distances*): PQ distances and the best top_k over each query's
own list of ids.

GPU: strictly (ids and distance bits) against the exact-rational reference of tests/_numeric_edges.py and against
query_batch / query_batch_filtered on the same handle; shapes around the workgroup of 256 candidates, the sort's 16384 and
the slice of 2^20; the id rules; shards; the tables forms; the distance form; the state a call leaves behind.  CPU: the
symbols, the hand-derived separation of the two sum rules, the id classification, de-duplication and padding, the argument
checks.  Nothing is skipped and no case is exempt.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _candidates_restatement as C
import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_candidate_search", "dpq_candidate_search_device", "dpq_candidate_search_tables",
           "dpq_candidate_search_device_tables", "dpq_candidate_distances", "dpq_candidate_distances_device")
_cache = {}


def built_class(name, M=8, n=ne.N_SCAN):
    """One build per (class, M, n) and module; nobody writes to it."""
    key = (name, M, n)
    if key not in _cache:
        c = ne.build_class(name, M, 256, n, plain_rule=(M, n) == (8, ne.N_SCAN))
        c["luts"] = np.stack([ne.np_table(t) for t in c["tables"]])
        _cache[key] = c
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
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def open_class(api, c, plain=False, **opts):
    if plain:
        idx = api.DeltaPQIndex.open_plain(c["codes"], K=c["K"], **opts)
    else:
        idx = api.DeltaPQIndex.open_memory(c["payload"], c["n"], c["M"], c["K"], **opts)
    return idx.set_codebook(c["cb"])


def padded(lists, n_cand=None, fill=-1):
    """int32 [len(lists)][n_cand]: ragged lists padded with -1."""
    n_cand = max(1, max(len(l) for l in lists)) if n_cand is None else n_cand
    out = np.full((len(lists), n_cand), fill, dtype=np.int32)
    for q, l in enumerate(lists):
        out[q, :len(l)] = l
    return out


def restated(alld, use, cand, k, **ids):
    return [C.search_row(alld[u], cand[q], k, **ids) for q, u in enumerate(use)]


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_the_six_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert "int %s(" % name in header, name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in bound and hasattr(lib, name), name + " is not bound"


def test_the_two_sum_rules_separate_on_a_hand_derived_node():
    """T[0] = 2^24, T[1] = 1, T[2] = 1, the rest 0.  The DTC rule: 16777218 exactly, an fp32 value.  The plain rule:
    2^24 + 1 is a tie and goes to the even 2^24, and so again."""
    table = np.zeros((8, 256), dtype=np.float32)
    table[0, 9], table[1, 9], table[2, 9] = 2.0 ** 24, 1.0, 1.0
    code = np.array([[9, 9, 9, 0, 0, 0, 0, 0]], dtype=np.uint8)
    assert bits(C.distances(table, code, plain=False))[0] == 0x4B800001
    assert bits(C.distances(table, code, plain=True))[0] == 0x4B800000
    row = C.search_row(C.distances(table, code, plain=False), [0], 1, even_rule=False)
    assert row[0][0] == 0 and bits(row[1])[0] == 0x4B800001


def test_id_classification():
    L, S, X = C.LOCAL, C.SKIP, C.NONE
    cls, local = C.classify([10, 9, 11, 0, 8, -1, -7], 0, 10, 10, True)          # N = 10, DTC
    assert cls.tolist() == [L, X, X, L, L, S, S] and local.tolist() == [9, -1, -1, 0, 8, -1, -1]
    cls, local = C.classify([10, 11, 9], 0, 11, 11, True)                        # N = 11, DTC
    assert cls.tolist() == [L, X, L] and local.tolist() == [10, -1, 9]
    cls, local = C.classify([9, 10], 0, 10, 10, False)                           # a plain handle, N = 10
    assert cls.tolist() == [L, X] and local.tolist() == [9, -1]
    cls, local = C.classify([4, 10, 5, 9, 8, 11], 5, 5, 10, True)                # the shard [5, 10) of N = 10
    assert cls.tolist() == [S, L, L, X, L, X] and local.tolist() == [-1, 4, 0, -1, 3, -1]
    cls, _ = C.classify([4, 5, 10, 9], 0, 5, 10, True)                           # ... and the shard [0, 5)
    assert cls.tolist() == [L, S, S, X]
    with pytest.raises(ValueError):
        C.candidate_distances(np.zeros(10, dtype=np.float32), [9])


def test_a_node_named_twice_counts_once_and_rows_are_padded():
    d = np.arange(10, dtype=np.float32)[::-1].copy()                             # node i at distance 9 - i
    ids, dist = C.search_row(d, [3, -1, 3, 7], 3, even_rule=False)
    assert ids.tolist() == [7, 3, -1] and dist[:2].tolist() == [2.0, 6.0] and np.isposinf(dist[2])
    got = C.candidate_distances(d, [3, -1, 3, 7], even_rule=False)
    assert got[[0, 2, 3]].tolist() == [6.0, 6.0, 2.0] and np.isnan(got[1])


def test_argument_errors_need_no_device(lib):
    """NULL pointers and the bounds of top_k and n_cand are refused before the handle is looked at (the handle below is
    never dereferenced) and before a device is asked for."""
    buf = np.zeros(8 * 256, dtype=np.float32)
    ib = np.zeros(64, dtype=np.int32)
    p, ip, h = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ib.ctypes.data), ctypes.c_void_p(0x1000)
    for fn in (lib.dpq_candidate_search, lib.dpq_candidate_search_tables):
        assert fn(None, p, 1, ip, 4, 2, ip, p) == ERR_ARG
        assert fn(h, None, 1, ip, 4, 2, ip, p) == ERR_ARG
        assert fn(h, p, 1, None, 4, 2, ip, p) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 2, None, p) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 2, ip, None) == ERR_ARG
        assert fn(h, p, -1, ip, 4, 2, ip, p) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 0, ip, p) == ERR_ARG            # top_k < 1
        assert fn(h, p, 1, ip, 4, 5, ip, p) == ERR_ARG            # top_k > n_cand
        assert fn(h, p, 1, ip, 16385, 2, ip, p) == ERR_ARG        # n_cand > 16384
        assert fn(h, p, 0, ip, 4, 5, ip, p) == ERR_ARG            # ... also where there is no query
    for fn in (lib.dpq_candidate_search_device, lib.dpq_candidate_search_device_tables):
        assert fn(None, p, 1, ip, 4, 2, ip, p, None) == ERR_ARG
        assert fn(h, None, 1, ip, 4, 2, ip, p, None) == ERR_ARG
        assert fn(h, p, 1, None, 4, 2, ip, p, None) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 2, None, p, None) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 2, ip, None, None) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 0, ip, p, None) == ERR_ARG
        assert fn(h, p, 1, ip, 4, 5, ip, p, None) == ERR_ARG
        assert fn(h, p, 1, ip, 16385, 2, ip, p, None) == ERR_ARG
    assert lib.dpq_candidate_distances(None, p, 1, ip, 4, p) == ERR_ARG
    assert lib.dpq_candidate_distances(h, None, 1, ip, 4, p) == ERR_ARG
    assert lib.dpq_candidate_distances(h, p, 1, None, 4, p) == ERR_ARG
    assert lib.dpq_candidate_distances(h, p, 1, ip, 4, None) == ERR_ARG
    assert lib.dpq_candidate_distances(h, p, 1, ip, 0, p) == ERR_ARG
    assert lib.dpq_candidate_distances(h, p, 1, ip, 16385, p) == ERR_ARG
    assert lib.dpq_candidate_distances_device(None, p, 1, ip, 4, p, None) == ERR_ARG
    assert lib.dpq_candidate_distances_device(h, p, 1, ip, 0, p, None) == ERR_ARG
    assert lib.dpq_candidate_distances_device(h, p, 1, ip, 16385, p, None) == ERR_ARG
    assert b"dpq_candidate_distances_device" in lib.dpq_last_error()


# ---- 1. against the exact-rational reference ---------------------------------------------------------------------------------

HANDLES = {"dtc_m8": (8, False), "dtc_m16": (16, False), "plain_m8": (8, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", ["fp32_ties", "overflow"])
def test_all_ids_as_candidates_against_the_exact_reference(gpu, name, handle, nq):
    """Every id of the index, in an order of the query's own, padded to 4100: the answer is the index's top-k -- by the
    DTC rule on the DTC handles, by the plain rule on the plain one (fp32_ties tells them apart), +inf included."""
    M, plain = HANDLES[handle]
    c = built_class(name, M)
    n, U = c["n"], len(c["queries"])
    alld = c["d32"] if plain else c["d64"]
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    rng = np.random.default_rng(100 + nq)
    cand = padded([rng.permutation(n) for _ in range(nq)], n_cand=4100)
    with open_class(gpu, c, plain) as idx:
        for k in (1, 10, 1000):
            what = "%s %s nq=%d top-%d" % (name, handle, nq, k)
            got = idx.candidate_search(qs, cand, k)
            om._rows_equal(got, [ne.topk(alld[u], k) for u in use], what)
            om._rows_equal(got, restated(alld, use, cand, k, even_rule=not plain), what + " (restatement)")
            assert same(got, idx.query_batch(qs, k)), what + ": differs from query_batch on this handle"


# ---- 2. per-query subsets -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["half", "one_percent", "fewer_than_top_k"])
def test_per_query_subsets(gpu, kind):
    c = built_class("fp32_ties")
    n, U, nq, k = c["n"], len(c["queries"]), 33, 10
    alld = c["d64"]
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    rng = np.random.default_rng(7)
    if kind == "fewer_than_top_k":
        masks = np.zeros((nq, n), dtype=bool)
        for q in range(nq):
            masks[q, rng.choice(n, size=q % k, replace=False)] = True          # 0 .. 9 valid ids
    else:
        masks = rng.random((nq, n)) < (0.5 if kind == "half" else 0.01)
    lists = [rng.permutation(np.flatnonzero(m)) for m in masks]
    cand = padded(lists, n_cand=max(k + 2, max(len(l) for l in lists)))
    assert (kind == "fewer_than_top_k") == all(len(l) < k for l in lists)
    with open_class(gpu, c) as idx:
        got = idx.candidate_search(qs, cand, k)
        om._rows_equal(got, [ne.topk(alld[u], k, masks[q]) for q, u in enumerate(use)], kind)
        for q in (0, 16, 32):
            with gpu.IdFilter.from_mask(idx, masks[q]) as f:
                want = idx.query_batch_filtered(qs[q:q + 1], k, f)
            assert same((got[0][q:q + 1], got[1][q:q + 1]), want), "%s query %d: differs from query_batch_filtered" % (kind, q)


# ---- 3. shapes ----------------------------------------------------------------------------------------------------------------------

def _messy_lists(rng, nq, n_cand, n):
    """Random ids with repeats, and padding in the middle of every list that has a middle."""
    cand = rng.integers(0, n, size=(nq, n_cand)).astype(np.int32)
    if n_cand >= 3:
        cand[:, 1::7] = -1
        cand[:, 2::5] = cand[:, :1]                                            # the first id again and again
    return cand


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand", [1, 255, 256, 257])
def test_shapes_around_the_workgroup(gpu, n_cand):
    c = built_class("fp32_ties")
    n, U, nq = c["n"], len(c["queries"]), 5
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    cand = _messy_lists(np.random.default_rng(n_cand), nq, n_cand, n)
    with open_class(gpu, c) as idx:
        for k in sorted({1, min(10, n_cand), n_cand}):
            om._rows_equal(idx.candidate_search(qs, cand, k), restated(c["d64"], use, cand, k), "n_cand=%d top-%d" % (n_cand, k))


@pytest.mark.gpu
def test_the_longest_lists_over_more_than_one_slice(gpu):
    """65 queries of 16384 candidates are 1 064 960 candidates: a slice of 64 queries and one of one.  top_k == n_cand."""
    c = built_class("fp32_ties", 8, ne.N_BOOT)
    n, U, nq, n_cand = c["n"], len(c["queries"]), 65, 16384
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    cand = _messy_lists(np.random.default_rng(5), nq, n_cand, n)
    assert nq * n_cand > 1 << 20
    with open_class(gpu, c) as idx:
        want = restated(c["d64"], use, cand, n_cand)
        got = idx.candidate_search(qs, cand, n_cand)
        for q in (63, 64):                                                      # both sides of the slice boundary, by name
            om._rows_equal((got[0][q:q + 1], got[1][q:q + 1]), want[q:q + 1], "query %d at the slice boundary" % q)
        om._rows_equal(got, want, "n_cand=16384 top-16384")
        om._rows_equal(idx.candidate_search(qs, cand, 10), restated(c["d64"], use, cand, 10), "n_cand=16384 top-10")


# ---- 4. id rules on the device -------------------------------------------------------------------------------------------------------

def _generic_index(n, seed):
    """(payload, codes, cb, qs, d [nq][n] by the DTC rule, d by the plain rule) of a seeded index under SIFT-shaped tables."""
    from deltapq_amd import synth
    tree = ne.plain_tree(n, 8, 256, seed)
    payload, _ = synth.encode_dtc(tree)
    codes = synth.decode_tree_codes(tree)
    cb = synth.make_codebook(8, 256, 16, seed + 1)
    qs = synth.make_queries(3, 128, seed + 2)
    tabs = T.l2_tables(cb, qs)
    d64 = np.stack([C.distances(t, codes, plain=False) for t in tabs])
    d32 = np.stack([C.distances(t, codes, plain=True) for t in tabs])
    return payload, codes, cb, qs, d64, d32


def _both_forms(api, idx, qs, cand, k):
    """The host form's and the device form's outcome of one call: ("ok", ids, dists) or ("error", status)."""
    import torch
    out = []
    for form in ("host", "device"):
        try:
            if form == "host":
                ids, d = idx.candidate_search(qs, cand, k)
            else:
                ids, d = idx.candidate_search_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(cand).cuda(), k)
                ids, d = ids.cpu().numpy(), d.cpu().numpy()
            out.append(("ok", ids, d))
        except api.DpqError as e:
            out.append(("error", e.status))
    return out


def _refused(api, idx, qs, cand, k, what):
    for form, res in zip(("host", "device"), _both_forms(api, idx, qs, cand, k)):
        assert res == ("error", ERR_ARG), "%s, %s form: %r" % (what, form, res[:2])


def _answered(api, idx, qs, cand, k, want, what):
    for form, res in zip(("host", "device"), _both_forms(api, idx, qs, cand, k)):
        assert res[0] == "ok", "%s, %s form: status %r" % (what, form, res[1])
        om._rows_equal(res[1:], want, "%s, %s form" % (what, form))


@pytest.mark.gpu
def test_id_rules_on_the_device(gpu):
    base = np.array([[0, 5, -1, 77]] * 3, dtype=np.int32)

    def with_id(i):
        c = base.copy()
        c[1, 2] = i                                                             # in query 1, where the padding was
        return c

    # an even-N DTC index: N names the last node, N - 1 and N + 1 name nothing
    N = 4098
    payload, codes, cb, qs, d64, d32 = _generic_index(N, 31)
    with gpu.DeltaPQIndex.open_memory(payload, N, 8, 256).set_codebook(cb) as idx:
        want = [C.search_row(d64[q], with_id(N)[q], 4, n_total=N, n_local=N, even_rule=True) for q in range(3)]
        assert want[1][0].tolist().count(N) == 1
        _answered(gpu, idx, qs, with_id(N), 4, want, "even N, id N")
        _refused(gpu, idx, qs, with_id(N - 1), 4, "even N, id N - 1")
        _refused(gpu, idx, qs, with_id(N + 1), 4, "even N, id N + 1")
        _answered(gpu, idx, qs, with_id(N), 4, want, "even N, id N, after refused calls")
    # a plain handle over the same codes: N - 1 is a node like any other, N names nothing
    with gpu.DeltaPQIndex.open_plain(codes, K=256).set_codebook(cb) as idx:
        want = [C.search_row(d32[q], with_id(N - 1)[q], 4, even_rule=False) for q in range(3)]
        _answered(gpu, idx, qs, with_id(N - 1), 4, want, "plain, id N - 1")
        _refused(gpu, idx, qs, with_id(N), 4, "plain, id N")
    # an odd-N DTC index: N - 1 is the last node, N names nothing
    N = 4097
    payload, codes, cb, qs, d64, _ = _generic_index(N, 32)
    with gpu.DeltaPQIndex.open_memory(payload, N, 8, 256).set_codebook(cb) as idx:
        want = [C.search_row(d64[q], with_id(N - 1)[q], 4, even_rule=True) for q in range(3)]
        _answered(gpu, idx, qs, with_id(N - 1), 4, want, "odd N, id N - 1")
        _refused(gpu, idx, qs, with_id(N), 4, "odd N, id N")


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_shards_take_the_same_lists_and_merge(gpu):
    c = built_class("fp32_ties")
    n, U, nq = c["n"], len(c["queries"]), 9
    alld = c["d64"]
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    rng = np.random.default_rng(3)
    cand = padded([rng.permutation(n)[:3000] for _ in range(nq)], n_cand=3010)
    masks = np.zeros((nq, n), dtype=bool)
    for q in range(nq):
        masks[q, cand[q][cand[q] >= 0]] = True
    shards = [open_class(gpu, c, shard_rank=r, shard_count=2) for r in range(2)]
    try:
        bounds = [(s.info()["node_lo"], s.info()["node_hi"]) for s in shards]
        assert bounds[0][0] == 0 and bounds[0][1] == bounds[1][0] and bounds[1][1] == n and 0 < bounds[0][1] < n
        for k in (10, 1000):
            parts = [s.candidate_search(qs, cand, k) for s in shards]
            for r, (lo, hi) in enumerate(bounds):
                ids = dict(id_base=lo, n_local=hi - lo, n_total=n)
                want = [C.search_row(alld[u][lo:hi], cand[q], k, **ids) for q, u in enumerate(use)]
                om._rows_equal(parts[r], want, "shard %d top-%d" % (r, k))
            merged = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
            om._rows_equal(merged, [ne.topk(alld[u], k, masks[q]) for q, u in enumerate(use)], "merged top-%d" % k)
        # a list of the other shard's nodes alone comes back as padding
        lo1, hi1 = bounds[1]
        other = padded([np.arange(lo1, min(hi1, lo1 + 40))] * nq, n_cand=48)
        ids, d = shards[0].candidate_search(qs, other, 10)
        assert np.all(ids == -1) and np.all(np.isposinf(d))
        got = shards[1].candidate_search(qs, other, 10)
        assert np.all(got[0] >= lo1)
        # the distance form: NaN exactly at padding and at the other shard's entries
        for r, (lo, hi) in enumerate(bounds):
            dist = shards[r].candidate_distances(qs, cand)
            here = (cand >= lo) & (cand < hi)
            assert np.array_equal(np.isnan(dist), ~here), "shard %d: NaN where the entry is not this shard's" % r
            for q, u in enumerate(use):
                assert np.array_equal(bits(dist[q][here[q]]), bits(alld[u][cand[q][here[q]]])), "shard %d query %d" % (r, q)
    finally:
        for s in shards:
            s.close()


# ---- 6. tables forms ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_tables_forms(gpu):
    import torch
    c = built_class("fp32_ties")
    n, U, nq, k = c["n"], len(c["queries"]), 9, 10
    alld = c["d64"]
    use = np.arange(nq) % U
    qs, tabs = np.ascontiguousarray(c["queries"][use]), np.ascontiguousarray(c["luts"][use])
    rng = np.random.default_rng(11)
    cand = padded([rng.permutation(n)[:500] for _ in range(nq)], n_cand=512)
    want = restated(alld, use, cand, k)
    with gpu.DeltaPQIndex.open_memory(c["payload"], n, 8, 256) as idx:
        # before dpq_set_codebook: the tables forms work, the query forms are a state error
        om._rows_equal(idx.candidate_search_tables(tabs, cand, k), want, "tables, no codebook")
        ids, d = idx.candidate_search_tables_torch(torch.from_numpy(tabs).cuda(), torch.from_numpy(cand).cuda(), k)
        om._rows_equal((ids.cpu().numpy(), d.cpu().numpy()), want, "device tables, no codebook")
        for call in (lambda: idx.candidate_search(qs, cand, k), lambda: idx.candidate_distances(qs, cand)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == ERR_STATE
        idx.set_codebook(c["cb"])
        by_q = idx.candidate_search(qs, cand, k)
        om._rows_equal(by_q, want, "queries")
        assert same(idx.candidate_search_tables(tabs, cand, k), by_q), "tables of the queries differ from the queries"
        # an entry that is no distance: the status query_batch_tables gives it, from both forms
        bad = tabs.copy()
        bad[3, 2, 17] = -1.0
        with pytest.raises(gpu.DpqError) as ref:
            idx.query_batch_tables(bad, k)
        with pytest.raises(gpu.DpqError) as ref_dev:
            idx.query_batch_tables_torch(torch.from_numpy(bad).cuda(), k)
        with pytest.raises(gpu.DpqError) as e:
            idx.candidate_search_tables(bad, cand, k)
        assert e.value.status == ref.value.status == ERR_ARG
        with pytest.raises(gpu.DpqError) as e:
            idx.candidate_search_tables_torch(torch.from_numpy(bad).cuda(), torch.from_numpy(cand).cuda(), k)
        assert e.value.status == ref_dev.value.status == ERR_ARG
        om._rows_equal(idx.candidate_search_tables(tabs, cand, k), want, "tables after a refused call")
        # inner product composes: the gaps tables over every id are query_batch_tables' answer, and score from there
        ip_tabs, bias = idx.ip_tables(qs)
        everything = padded([rng.permutation(n) for _ in range(nq)])
        gaps = idx.candidate_search_tables(ip_tabs, everything, k)
        assert same(gaps, idx.query_batch_tables(ip_tabs, k)), "inner-product tables: differs from query_batch_tables"
        ids_ip, scores, _, _ = idx.query_batch_ip(qs, k)
        assert np.array_equal(gaps[0], ids_ip) and np.array_equal(bits(gpu.ip_scores(bias, gaps[1], gaps[0])), bits(scores))


# ---- 7. distances form ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
def test_distances_in_place(gpu, handle):
    import torch
    M, plain = HANDLES[handle]
    c = built_class("overflow", M)
    n, U, nq = c["n"], len(c["queries"]), 7
    alld = c["d32"] if plain else c["d64"]
    use = np.arange(nq) % U
    qs = np.ascontiguousarray(c["queries"][use])
    cand = _messy_lists(np.random.default_rng(13), nq, 600, n)
    with open_class(gpu, c, plain) as idx:
        got = idx.candidate_distances(qs, cand)
        assert got.shape == cand.shape and np.array_equal(np.isnan(got), cand < 0)
        for q, u in enumerate(use):
            real = cand[q] >= 0
            assert np.array_equal(bits(got[q][real]), bits(alld[u][cand[q][real]])), "query %d" % q
            assert np.all(bits(got[q][~real]) == 0x7FC00000)
        assert np.isposinf(got[cand >= 0]).any()                                 # +inf is an ordinary value
        dev = idx.candidate_distances_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(cand).cuda())
        assert np.array_equal(bits(dev.cpu().numpy()), bits(got))


# ---- 8. state and faces ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_state_and_faces(gpu):
    import torch
    c = built_class("fp32_ties")
    n, U, nq, k = c["n"], len(c["queries"]), 65, 10
    alld = c["d64"]
    use = np.arange(nq) % U
    other = (use + 1) % U                                                        # the candidate call asks about ANOTHER query
    qs, qo = np.ascontiguousarray(c["queries"][use]), np.ascontiguousarray(c["queries"][other])
    rng = np.random.default_rng(17)
    cand = padded([rng.permutation(n)[:700] for _ in range(nq)], n_cand=701)
    want = restated(alld, other, cand, k)
    with open_class(gpu, c, batch_decode=1) as idx:
        first = idx.query_batch(qs, k)
        om._rows_equal(first, [ne.topk(alld[u], k) for u in use], "query_batch, first")
        host = idx.candidate_search(qo, cand, k)
        om._rows_equal(host, want, "host form")
        assert same(idx.query_batch(qs, k), first), "query_batch changed after a candidate call"
        ids, d = idx.candidate_search_torch(torch.from_numpy(qo).cuda(), torch.from_numpy(cand).cuda(), k)
        assert same((ids.cpu().numpy(), d.cpu().numpy()), host), "the torch form differs from the host form"
        idx.candidate_distances(qo, cand)
        idx.candidate_search_tables(np.ascontiguousarray(c["luts"][other]), cand, k)
        assert same(idx.query_batch(qs, k), first), "query_batch changed after the other candidate calls"
        # no query is no work, and no error
        e = idx.candidate_search(np.zeros((0, 8), dtype=np.float32), np.zeros((0, 4), dtype=np.int32), 2)
        assert e[0].shape == (0, 2)
        # a rotated index rotates the queries and nothing else
        rot = np.linalg.qr(rng.normal(size=(8, 8)))[0].astype(np.float32)
        r = gpu.RotatedIndex(idx, rot)
        by_hand = gpu.rotate(qo, rot)
        assert same(r.candidate_search(qo, cand, k), idx.candidate_search(by_hand, cand, k))
        ids, d = r.candidate_search_torch(torch.from_numpy(qo).cuda(), torch.from_numpy(cand).cuda(), k)
        assert same((ids.cpu().numpy(), d.cpu().numpy()), idx.candidate_search(by_hand, cand, k))
        assert np.array_equal(bits(r.candidate_distances(qo, cand)), bits(idx.candidate_distances(by_hand, cand)))
