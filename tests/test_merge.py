"""The top-k merge (dpq_merge_topk_host, dpq_merge_topk_device, dpq_merge_topk_device_packed; merge_kernel)
on hand-built partial lists.

tests/_merge_cases.py holds the case table (fixed and seeded; each pytest id spells out n_lists, top_k, nq, the fill kind
and the seed), the reference (plain numpy: the valid rows of all lists, np.lexsort by (distance bits, id), the first
top_k, padding) and the kernel's rank rule restated with np.searchsorted.  Every comparison is bit equality of ids and
distance bit patterns, every query of every case.

CPU: the reference on a hand-written case; the host merge against the reference over the whole table, also with every
list shuffled; the restated rank rule reproduces the reference on every case -- the stable rule everywhere, the strict rule
the kernel had on every case without repeated keys, while on every `dups` case the strict rule leaves a hole (which is
how the `dups` GPU cases are known to fail on the kernel as it was); every fill kind holds what its name claims; argument
errors and nq == 0 of all three calls, answered before any device call; pack_lists / unpack_lists keep bit patterns.

GPU: merge_topk_torch and merge_topk_packed_torch (the packed tensor built by dist.pack_lists) against the reference
over the whole table, into outputs pre-filled with a sentinel; one shape per fill kind on a non-default stream; nq == 0;
and the five shards of a 20 001-code index at top_k = 300 through the host, device and packed device merge."""
import ctypes

import numpy as np
import pytest

import _merge_cases as mc

f32 = np.float32
OK, ERR_ARG = 0, -1
INF = float("inf")


def assert_rows(got, want, what):
    gi, gd = np.asarray(got[0]), np.asarray(got[1])
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape and gi.dtype == np.int32 and gd.dtype == f32, what
    bad = np.flatnonzero((gi != wi).any(axis=1) | (mc.bits_of(gd) != mc.bits_of(wd)).any(axis=1))
    if len(bad):
        q = int(bad[0])
        r = int(np.flatnonzero((gi[q] != wi[q]) | (mc.bits_of(gd[q]) != mc.bits_of(wd[q])))[0])
        raise AssertionError("%s: %d of %d queries differ; query %d from rank %d on\n got  %s %s\n want %s %s" % (
            what, len(bad), len(gi), q, r, gi[q, r:r + 6], gd[q, r:r + 6], wi[q, r:r + 6], wd[q, r:r + 6]))


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_table_is_what_the_issue_says():
    T = mc.TABLE
    ids = [mc.case_id(c) for c in T]
    assert len(set(ids)) == len(ids)
    assert mc._build_table() == T                                       # fixed: the same table every time
    shapes_of = {}
    for c in T:
        shapes_of.setdefault(c["fill"], set()).add((c["n_lists"], c["top_k"], c["nq"]))
    assert set(shapes_of) == {"full", "ragged", "short", "all_empty", "ties", "interleaved", "one_wins_first",
                              "one_wins_last", "edges_of_value", "dups"}
    for fill, shapes in shapes_of.items():
        assert len(shapes) >= 4, fill
    for fill in ("dups", "ties", "ragged"):
        assert {(8, 2048, 2), (16, 1024, 2)} <= shapes_of[fill], fill
    assert set().union(*shapes_of.values()) == {
        (1, 1, 1), (1, 2048, 3), (2, 1, 5), (3, 7, 65), (2, 511, 2), (2, 512, 2), (2, 513, 2), (5, 257, 4), (8, 100, 33),
        (8, 2048, 2), (16, 1024, 2), (7, 2340, 1), (16384, 1, 2), (4, 300, 1000)}
    assert all(c["n_lists"] * c["top_k"] <= 16384 for c in T)
    ids_a, dists_a, _ = mc.build_lists(T[0])
    assert not ids_a.flags.writeable and not dists_a.flags.writeable    # shared, never changed


def test_reference_on_a_hand_written_case():
    """3 lists x top_k 4 x 2 queries.  Query 0: 1.0 ties across lists 0 and 1 (id 3 before id 5), list 1 is short, list 2
    repeats 2.0 and its lower id makes the cut.  Query 1: list 0 is empty, the one +inf row is valid and precedes the
    padding; a padding row's id and distance do not matter."""
    ids = np.array([[[5, 1, 9, 2], [-1, -1, -1, -1]],
                    [[3, 7, -1, -1], [11, -1, -1, -1]],
                    [[8, 0, 4, 6], [2, -7, -1, -1]]], dtype=np.int32)
    dists = np.array([[[1.0, 2.0, 3.0, 4.0], [INF, INF, INF, INF]],
                      [[1.0, 2.5, INF, INF], [7.0, INF, INF, INF]],
                      [[0.5, 2.0, 2.0, 9.0], [INF, 0.25, INF, INF]]], dtype=f32)
    want_i = [[8, 3, 5, 0], [11, 2, -1, -1]]
    want_d = [[0.5, 1.0, 1.0, 2.0], [7.0, INF, INF, INF]]
    for got in (mc.reference(ids, dists), mc.rank_rule(ids, dists, stable=True), mc.rank_rule(ids, dists, stable=False)):
        assert got[0].dtype == np.int32 and got[1].dtype == f32
        assert got[0].tolist() == want_i and got[1].tolist() == want_d, got
    # the same key in lists 0 and 2: kept twice by the reference and the stable rule; the strict rule gives both copies
    # rank 2 and leaves rank 3 as padding
    ids2, dists2 = ids.copy(), dists.copy()
    ids2[2, 0], dists2[2, 0] = [8, 5, 4, 6], [0.5, 1.0, 2.0, 9.0]
    for got in (mc.reference(ids2, dists2), mc.rank_rule(ids2, dists2, stable=True)):
        assert got[0][0].tolist() == [8, 3, 5, 5] and got[1][0].tolist() == [0.5, 1.0, 1.0, 1.0], got
    old = mc.rank_rule(ids2, dists2, stable=False)
    assert old[0][0].tolist() == [8, 3, 5, -1] and old[1][0].tolist() == [0.5, 1.0, 1.0, INF]
    assert mc.has_hole(old[0], mc.reference(ids2, dists2)[0])
    ids2[0, 0, 0] = 6                                                   # no longer a repeat: (1.0, 6) against (1.0, 5)
    assert mc.rank_rule(ids2, dists2, stable=False)[0][0].tolist() == [8, 3, 5, 6]
    # a later key lands behind the hole: padding in the middle of the list
    ids3 = np.array([[[1, 3, 5]], [[1, 2, 4]]], np.int32)
    dists3 = np.array([[[1.0, 3.0, 5.0]], [[1.0, 2.0, 4.0]]], f32)
    assert mc.reference(ids3, dists3)[0].tolist() == [[1, 1, 2]]
    assert mc.rank_rule(ids3, dists3, stable=True)[0].tolist() == [[1, 1, 2]]
    old = mc.rank_rule(ids3, dists3, stable=False)
    assert old[0].tolist() == [[1, -1, 2]] and old[1].tolist() == [[1.0, INF, 2.0]]
    # keys order by the distance's BITS as uint32: -0.0 (0x80000000) sorts behind +inf (0x7f800000)
    got = mc.reference(np.array([[[4, 9]], [[6, -1]]], np.int32), np.array([[[INF, -0.0]], [[1.0, INF]]], f32))
    assert got[0].tolist() == [[6, 4]] and got[1].tolist() == [[1.0, INF]]


def _shuffled(ids, dists, seed):
    """Every list's rows in a random order (ids and distances together)."""
    rng = np.random.default_rng(seed)
    perm = np.argsort(rng.random(ids.shape), axis=2)
    return np.take_along_axis(ids, perm, axis=2), np.take_along_axis(dists, perm, axis=2)


@pytest.mark.parametrize("case", mc.TABLE, ids=mc.case_id)
def test_host_merge_equals_the_reference(lib, case):
    from deltapq_amd import api
    ids, dists, want = mc.build_lists(case)
    assert_rows(api.merge_topk_host(ids, dists), want, "host merge")
    # the host call sorts whatever it is given: the lists need not arrive sorted
    si, sd = _shuffled(ids, dists, case["seed"])
    if case["top_k"] > 1 and case["fill"] != "all_empty":
        assert not _sorted_with_padding_last(si, sd)
    assert_rows(api.merge_topk_host(si, sd), want, "host merge of unsorted lists")


def _sorted_with_padding_last(ids, dists):
    keys = mc.keys_of(ids, dists)
    return bool(np.all(keys[:, :, :-1] <= keys[:, :, 1:]))


@pytest.mark.parametrize("case", mc.TABLE, ids=mc.case_id)
def test_no_case_is_vacuous(case):
    """From the data and the restated rank rule alone: the lists meet the device calls' contract; the stable rule
    reproduces the reference; so does the strict rule where no key repeats, and on `dups` it leaves a hole in every
    query; and the fill kind holds what its name claims."""
    ids, dists, want = mc.build_lists(case)
    L, k, nq, fill = case["n_lists"], case["top_k"], case["nq"], case["fill"]
    what = mc.case_id(case)
    assert ids.shape == dists.shape == (L, nq, k)
    assert _sorted_with_padding_last(ids, dists), what
    valid = ids >= 0
    counts = valid.sum(axis=2)                                          # [n_lists][nq]
    total = counts.sum(axis=0)                                          # [nq]
    keys = mc.keys_of(ids, dists)
    n_keys = np.array([len(np.unique(keys[:, q][valid[:, q]])) for q in range(nq)])
    assert_rows(mc.rank_rule(ids, dists, stable=True), want, "the stable rank rule")
    old = mc.rank_rule(ids, dists, stable=False)
    if fill == "dups":
        assert L >= 2 and k >= 2
        assert np.all(n_keys < total), what
        for q in range(nq):
            assert mc.has_hole(old[0][q], want[0][q]), "%s query %d: the strict rule leaves no hole" % (what, q)
            K = keys[:, q]
            in_two = np.intersect1d(K[0][valid[0, q]], K[1][valid[1, q]])
            in_last = np.intersect1d(K[0][valid[0, q]], K[L - 1][valid[L - 1, q]])
            if q % 3 == 0:
                assert len(in_two) >= 1, what
            elif q % 3 == 1:
                assert all(len(np.intersect1d(in_two, K[l][valid[l, q]])) == len(in_two) >= 1 for l in range(L)), what
            else:
                own = K[0][valid[0, q]]
                assert np.any(own[:-1] == own[1:]) and len(in_last) >= 1, what
    else:
        assert np.all(n_keys == total), "%s: a repeated key outside `dups`" % what
        assert_rows(old, want, "the strict rank rule")
    if fill in ("full", "ties", "interleaved", "one_wins_first", "one_wins_last"):
        assert np.all(counts == k), what
    if fill == "ragged":
        assert np.all(counts.min(axis=0) == 0) and np.all(counts.max(axis=0) == k), what
        assert L == 2 or k == 1 or len(np.unique(counts)) > 2, what
    if fill == "short":
        assert np.all(total < k), what
        assert np.all(total >= 1) or k == 1, what
        assert np.all(want[0][:, -1] == -1) and np.all(np.isposinf(want[1][:, -1])), what
    if fill == "all_empty":
        assert total.sum() == 0 and np.all(want[0] == -1) and np.all(np.isposinf(want[1])), what
    if fill == "ties":
        assert set(np.unique(mc.bits_of(dists))) <= set(mc.TIE_POOL.tolist()), what
        assert len(np.unique(mc.bits_of(dists)[:, 0])) == 1, what
        assert nq == 1 or len(np.unique(mc.bits_of(dists))) == 3 or L * k < 8, what
        assert mc.ties_straddle(ids, dists, 0), what
        assert nq == 1 or L * k < 8 or any(mc.ties_straddle(ids, dists, q) for q in range(1, nq)), what
    if fill == "interleaved" and k > 1:
        # every search of a key in another list lands strictly inside it, except for the few keys at the global ends
        for q in range(min(nq, 3)):
            K = keys[:, q]
            inside = [0 < p < k for own in range(L) for l in range(L) if l != own
                      for p in np.searchsorted(K[l], K[own][1:-1]).tolist()]
            assert all(inside), what
    if fill in ("one_wins_first", "one_wins_last"):
        w = 0 if fill == "one_wins_first" else L - 1
        for q in range(nq):
            K = keys[:, q]
            for l in range(L):
                if l != w:
                    assert np.all(np.searchsorted(K[w], K[l]) == k) and np.all(np.searchsorted(K[l], K[w]) == 0), what
            assert np.array_equal(want[0][q], ids[w, q]), what
    if fill == "edges_of_value":
        b = mc.bits_of(dists)
        inf_valid = valid & (b == 0x7f800000)
        assert np.any(inf_valid) and np.any(ids == mc.ID_MAX), what
        assert np.any(valid & (b == 0)) or k == 1, what
        assert np.any(ids == 0) or L * k == 1, what
        # +inf rows that are valid reach the output ahead of the padding, ascending by id, and some are cut
        for q in range(nq):
            wi, wb = want[0][q], mc.bits_of(want[1][q])
            at_inf = np.flatnonzero((wi >= 0) & (wb == 0x7f800000))
            assert len(at_inf) >= 1 and np.all(np.diff(wi[at_inf]) > 0), what
            assert inf_valid[:, q].sum() > len(at_inf) or L == 1, what
        if L * k > 2:
            pad_i, pad_b = ids[~valid], b[~valid]
            assert np.any(pad_i == -1) and np.any(pad_i == -2**31) and np.any((pad_i < -2) & (pad_i > -2**31)), what
            assert np.any(pad_b == 0) and np.any(pad_b == 0x7fc00000) and np.any(pad_b == 0xbf800000), what


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_argument_errors_come_before_any_device_call(lib):
    """DPQ_ERR_ARG for a NULL pointer, n_lists < 1, top_k < 1, nq < 0 (all three calls) and for more than 16384 keys per
    query (the device calls), with or without a GPU: the arguments are checked before the device is touched.  The
    pointers of the device calls are never followed here."""
    ids = np.zeros((2, 3, 4), dtype=np.int32)
    dists = np.zeros((2, 3, 4), dtype=f32)
    packed = np.zeros((2, 3, 8), dtype=np.int32)
    oi, od = np.zeros((3, 4), dtype=np.int32), np.zeros((3, 4), dtype=f32)
    I, D, P, OI, OD = _ptr(ids), _ptr(dists), _ptr(packed), _ptr(oi), _ptr(od)

    def host(i=I, d=D, n_lists=2, nq=3, top_k=4, o_i=OI, o_d=OD):
        return lib.dpq_merge_topk_host(i, d, n_lists, nq, top_k, o_i, o_d)

    def device(i=I, d=D, n_lists=2, nq=3, top_k=4, o_i=OI, o_d=OD):
        return lib.dpq_merge_topk_device(i, d, n_lists, nq, top_k, o_i, o_d, 0, None)

    def device_packed(p=P, n_lists=2, nq=3, top_k=4, o_i=OI, o_d=OD):
        return lib.dpq_merge_topk_device_packed(p, n_lists, nq, top_k, o_i, o_d, 0, None)

    assert host() == OK
    for call in (host, device):
        for name in ("i", "d", "o_i", "o_d"):
            assert call(**{name: None}) == ERR_ARG, (call.__name__, name)
    for name in ("p", "o_i", "o_d"):
        assert device_packed(**{name: None}) == ERR_ARG, name
    for call in (host, device, device_packed):
        for bad in (dict(n_lists=0), dict(n_lists=-1), dict(top_k=0), dict(top_k=-3), dict(nq=-1)):
            assert call(**bad) == ERR_ARG, (call.__name__, bad)
    for call in (device, device_packed):
        for n_lists, top_k in ((16385, 1), (1, 16385), (5, 3277), (3277, 5)):     # 16385 keys: one past 128 KB of LDS
            assert n_lists * top_k == 16385
            assert call(n_lists=n_lists, top_k=top_k) == ERR_ARG, (call.__name__, n_lists, top_k)
        assert call(n_lists=2**20, top_k=2**20) == ERR_ARG                        # the product is taken in 64 bits
    # nq == 0 is no error and touches neither a device nor the outputs
    oi[:], od[:] = 77, 7.5
    assert host(nq=0) == OK and device(nq=0) == OK and device_packed(nq=0) == OK
    assert np.all(oi == 77) and np.all(od == 7.5)
    assert device(nq=0, n_lists=8, top_k=2048) == OK and device_packed(nq=0, n_lists=16384, top_k=1) == OK


def test_pack_and_unpack_keep_bit_patterns():
    import torch
    from deltapq_amd.dist import pack_lists, unpack_lists
    rng = np.random.default_rng(5)
    world, nq, k = 3, 4, 5
    bits = rng.integers(0, 2**32, size=(world, nq, k), dtype=np.uint64).astype(np.uint32)
    bits[0, 0] = [0x7fc00001, 0xffffffff, 0x7f800000, 0x80000000, 0x7f800001]   # quiet NaNs, +inf, -0.0, a signalling NaN
    bits[2, 3, :3] = [0xff800000, 0x00000001, 0x7fa00000]
    ids = rng.integers(-2**31, 2**31, size=(world, nq, k), dtype=np.int64).astype(np.int32)
    t_ids = torch.from_numpy(ids)
    t_d = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    rows = [pack_lists(t_ids[r], t_d[r]) for r in range(world)]
    assert all(r.shape == (nq, 2 * k) and r.dtype == torch.int32 and r.is_contiguous() for r in rows)
    assert np.array_equal(rows[1][:, :k].numpy(), ids[1]) and np.array_equal(rows[1][:, k:].numpy().view(np.uint32), bits[1])
    gi, gd = unpack_lists(torch.stack(rows), k)
    assert gi.dtype == torch.int32 and gd.dtype == torch.float32 and gi.shape == gd.shape == (world, nq, k)
    assert np.array_equal(gi.numpy(), ids)
    assert np.array_equal(gd.view(torch.int32).numpy().view(np.uint32), bits)
    # a non-contiguous slice packs like its copy
    wide_i, wide_d = torch.from_numpy(np.tile(ids[0], (1, 2))), torch.from_numpy(np.tile(bits[0].view(np.int32), (1, 2))).view(torch.float32)
    assert torch.equal(pack_lists(wide_i[:, :k], wide_d[:, :k]), rows[0])


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def _sentinel_out(nq, k):
    import torch
    oi = torch.full((nq, k), mc.SENTINEL_ID, dtype=torch.int32, device="cuda")
    od = torch.full((nq, k), mc.SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    return oi, od


def _device_merge(gpu, ids, dists, packed):
    """One device merge of numpy lists into sentinel-filled outputs, on torch's current stream; numpy results."""
    import torch
    from deltapq_amd.dist import pack_lists
    n_lists, nq, k = ids.shape
    t_ids, t_d = torch.tensor(ids, device="cuda"), torch.tensor(dists, device="cuda")
    out = _sentinel_out(nq, k)
    if packed:
        # every list's [nq][2k] rows as a rank packs them, all lists in one call
        gathered = pack_lists(t_ids.view(n_lists * nq, k), t_d.view(n_lists * nq, k)).view(n_lists, nq, 2 * k)
        got = gpu.merge_topk_packed_torch(gathered, k, out=out)
    else:
        got = gpu.merge_topk_torch(t_ids, t_d, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    torch.cuda.current_stream().synchronize()
    return got[0].cpu().numpy(), got[1].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", mc.TABLE, ids=mc.case_id)
def test_device_merge_equals_the_reference(gpu, case):
    ids, dists, want = mc.build_lists(case)
    assert_rows(_device_merge(gpu, ids, dists, packed=False), want, "dpq_merge_topk_device")


@pytest.mark.gpu
@pytest.mark.parametrize("case", mc.TABLE, ids=mc.case_id)
def test_packed_device_merge_equals_the_reference(gpu, case):
    ids, dists, want = mc.build_lists(case)
    assert_rows(_device_merge(gpu, ids, dists, packed=True), want, "dpq_merge_topk_device_packed")


def _one_per_fill():
    """Per fill kind its (8, 100, 33) case, or its (3, 7, 65) case where it has none."""
    out = []
    for fill in mc.FILLS:
        cases = [c for c in mc.TABLE if c["fill"] == fill]
        pick = [c for c in cases if (c["n_lists"], c["top_k"], c["nq"]) == (8, 100, 33)] or \
            [c for c in cases if (c["n_lists"], c["top_k"], c["nq"]) == (3, 7, 65)]
        out.append(pick[0])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", _one_per_fill(), ids=mc.case_id)
def test_device_merge_on_a_side_stream(gpu, case):
    import torch
    ids, dists, want = mc.build_lists(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for packed in (False, True):
            assert_rows(_device_merge(gpu, ids, dists, packed), want, "side stream, packed = %s" % packed)
    side.synchronize()


@pytest.mark.gpu
def test_device_merge_of_no_queries(gpu, lib):
    import torch
    k = 7
    ids = torch.empty((3, 0, k), dtype=torch.int32, device="cuda")
    for got in (gpu.merge_topk_torch(ids, torch.empty((3, 0, k), dtype=torch.float32, device="cuda")),
                gpu.merge_topk_packed_torch(torch.empty((3, 0, 2 * k), dtype=torch.int32, device="cuda"), k)):
        assert got[0].shape == (0, k) and got[1].shape == (0, k)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    # the C calls themselves, with real device pointers: DPQ_OK and the outputs untouched
    t_ids = torch.zeros((3, 2, k), dtype=torch.int32, device="cuda")
    t_d = torch.zeros((3, 2, k), dtype=torch.float32, device="cuda")
    packed = torch.zeros((3, 2, 2 * k), dtype=torch.int32, device="cuda")
    oi, od = _sentinel_out(2, k)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dpq_merge_topk_device(p(t_ids), p(t_d), 3, 0, k, p(oi), p(od), 0, stream) == OK
    assert lib.dpq_merge_topk_device_packed(p(packed), 3, 0, k, p(oi), p(od), 0, stream) == OK
    torch.cuda.synchronize()
    assert bool((oi == mc.SENTINEL_ID).all()) and bool((od.view(torch.int32) == mc.SENTINEL_BITS).all())


@pytest.mark.gpu
def test_five_shards_through_host_device_and_packed_merge(gpu):
    """n = 20 001 opened as 5 shards, top_k = 300, 33 queries (the shards of the option matrix): the same five partial
    lists through the three merges, bit-identical, and equal to the reference of this file."""
    import _option_matrix as om
    c = om.make_case(20001, nq=33, k=300, shards=5, seed=4242)
    inp = om.build_inputs(c)
    parts = []
    for rank in range(5):
        with gpu.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c, rank)) as idx:
            idx.set_codebook(inp["cb"])
            parts.append(idx.query_batch(inp["qs"], 300))
    ids = np.ascontiguousarray(np.stack([p[0] for p in parts]), dtype=np.int32)
    dists = np.ascontiguousarray(np.stack([p[1] for p in parts]), dtype=f32)
    assert ids.shape == (5, 33, 300) and np.all(ids >= 0)               # every shard holds more than 300 codes
    assert _sorted_with_padding_last(ids, dists)                        # what the shards deliver meets the contract
    want = mc.reference(ids, dists)
    host = gpu.merge_topk_host(ids, dists)
    assert_rows(host, want, "host merge of five shards")
    for packed in (False, True):
        got = _device_merge(gpu, ids, dists, packed)
        assert_rows(got, want, "device merge of five shards, packed = %s" % packed)
        assert np.array_equal(got[0], host[0]) and np.array_equal(mc.bits_of(got[1]), mc.bits_of(host[1]))
    assert len({int(np.argmax((ids[:, q] == want[0][q, 0]).any(axis=1))) for q in range(33)}) > 1   # the best come from several shards
