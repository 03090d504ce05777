"""IVF search by residual (dpq_ivf_search*_residual*) where its first suite (tests/test_ivf_residual.py) stops: sub-spaces
of more than one dwordx4, the scalar path at its smallest, top_k beyond 256 with the threshold refresh at every buffer size,
the device forms with a checked answer, calls cut into query slices and merged in rounds, groups with a ragged end.

Every comparison is strict -- ids equal, distances equal as fp32 bit patterns, padding -1 / +inf -- against
tests/_ivf_residual_restatement.py.  Nothing is skipped and no case is exempt.

Choices the issue leaves open, and why:
 * the refresh case is all whole numbers.  Its codebook is drawn from -3 .. 3 except cb[0][a] = (8 a, 0, 0, 0) and
   cb[1][b] = (b, 0, 0, 0); entry i of the long list has the code (i // 64, i % 64, 5, ...), the centroids and the two
   queries are whole numbers too, so every difference, square and sum is exact in fp32 and below 2^24 under both accumulate
   rules.  Query 0's residual is (900, ..) and (64, ..) in sub-spaces 0 and 1: its distance (900 - 8 a)^2 + (64 - b)^2 + c
   falls strictly with i (a step of a takes off at least 16 * 340 - 64 = 5376, more than the 4095 the wrap of b gives
   back).  Query 1's is (-300, ..), (-1, ..): (8 a + 300)^2 + (b + 1)^2 + c rises strictly (4864 against 4095).
 * the lists of 1024 hold 6000 plain codes; queries beyond the fifth repeat the first five, so that the restatement makes
   5 * 1024 tables once for the whole module.
"""
import numpy as np
import pytest

import _ivf_residual_restatement as RR
import test_ivf_residual as T

ERR_ARG = -1
F32 = np.float32
SHAPES = [(8, 8, 256), (8, 12, 200), (16, 8, 256), (16, 1, 256), (8, 1, 7)]
KS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
LONG, EQUAL = 4500, 1500
_cache = {}


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def refresh_case(plain):
    """Lists 0 (4500 entries, best last for query 0, best first for query 1), 1 (1500 entries of one code), 2 and 3 (50
    and 30 entries, 2000 away per dimension), 4 (the rest), 5 and 6 (empty); n = 6200 is even."""
    if ("refresh", plain) in _cache:
        return _cache["refresh", plain]
    from deltapq_amd import synth
    M, Ds, K, n = 8, 4, 256, 6200
    rng = np.random.default_rng(11)
    labels = rng.permutation(np.repeat(np.arange(5, dtype=np.int32), [LONG, EQUAL, 50, 30, n - LONG - EQUAL - 80]))
    codes = rng.integers(0, K, size=(n, M), dtype=np.uint8)
    i = np.arange(LONG)
    codes[labels == 0] = 5
    codes[labels == 0, 0], codes[labels == 0, 1] = i // 64, i % 64
    codes[labels == 1] = 9
    c = dict(M=M, Ds=Ds, K=K, plain=plain, n=n, lo=0, labels=labels, codes=codes)
    if not plain:
        depths = np.ones(n, dtype=np.uint8)
        depths[0] = 0
        tree = T.ne.tree_from_parts(codes[0], depths, np.ones((n, M), dtype=bool), codes, M)
        assert np.array_equal(synth.decode_tree_codes(tree), codes)
        c["payload"] = synth.encode_dtc(tree)[0]
    cb = rng.integers(-3, 4, size=(M, K, Ds)).astype(F32)
    cb[0], cb[1] = 0, 0
    cb[0, :, 0], cb[1, :, 0] = 8 * np.arange(K), np.arange(K)
    cents = rng.integers(-2, 3, size=(T.NLIST, M * Ds)).astype(F32)
    cents[2:4] += 2000
    r = np.zeros((2, M * Ds), dtype=F32)
    r[0, 0], r[0, Ds], r[1, 0], r[1, Ds] = 900, 64, -300, -1
    c.update(cb=cb, cents=cents, qs=(cents[0] + r).astype(F32))
    T.entries(c, labels, T.NLIST, codes)
    c["probes"] = np.array([[0, 1, 2, 3], [2, 0, 1, 3]], dtype=np.int32)
    c["want"] = RR.search_at(c, c["qs"], c["probes"], KS)
    c["alone"] = {l: RR.search_at(c, c["qs"], [[l], [l]], KS) for l in (0, 1, 2)}
    _cache["refresh", plain] = c
    return c


def lists_case():
    """6000 plain codes in 1024 lists, 5 % in none; five distinct queries."""
    if "lists" in _cache:
        return _cache["lists"]
    M, Ds, K, n, nlist = 8, 4, 256, 6000, 1024
    rng = np.random.default_rng(21)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    labels[rng.random(n) < 0.05] = -1
    c = dict(M=M, Ds=Ds, K=K, plain=True, n=n, lo=0, labels=labels, nlist=nlist, memo={},
             codes=rng.integers(0, K, size=(n, M), dtype=np.uint8), cb=rng.standard_normal((M, K, Ds)).astype(F32),
             cents=rng.standard_normal((nlist, M * Ds)).astype(F32), qs=rng.standard_normal((5, M * Ds)).astype(F32))
    T.entries(c, labels, nlist, c["codes"])
    _cache["lists"] = c
    return c


def open_lists(api, c):
    idx = api.DeltaPQIndex.open_plain(c["codes"], K=c["K"])
    idx.set_codebook(c["cb"])
    return idx, api.IVF.from_labels(idx, c["labels"], c["nlist"], centroids=c["cents"])


def prefixes(nq, nlist, nprobe, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int32)


def device(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(got):
    return got[0].cpu().numpy(), got[1].cpu().numpy()


def refused_in_the_last_row(api, ivf, qs, probes, nlist, k, want, what):
    """A probe >= nlist in the LAST row only, through the device form: DPQ_ERR_ARG, and the next call answers as before."""
    import torch
    bad = probes.copy()
    bad[-1, -1] = nlist
    t_q, t_bad, t_p = device(torch, qs, bad, probes)
    with pytest.raises(api.DpqError) as e:
        ivf.search_probes_residual_torch(t_q, t_bad, k)
    assert e.value.status == ERR_ARG, what
    assert RR.same(host(ivf.search_probes_residual_torch(t_q, t_p, k)), want), what + ": the call after the refused one"


# ---- CPU: what the shapes below rest on --------------------------------------------------------------------------------------

def slices_of(nq, nprobe, top_k):
    """(per, round) of include/deltapq_amd.h's limits: 2048 queries and 256 MiB of partial answers per slice, 16 384 keys
    per merge."""
    return max(1, min(nq, 2048, (256 << 20) // (nprobe * top_k * 8))), 16384 // top_k


MERGE_CALLS = [(2048, 8), (2048, 9), (17, 964), (2047, 1024)]


def test_the_shapes_cross_the_edges_they_are_chosen_for():
    assert slices_of(2049, 2, 3) == (2048, 5461) and slices_of(33, 1024, 2048) == (16, 8) and 33 - 2 * 16 == 1
    rounds = {(k, p): slices_of(5, p, k)[1] for k, p in MERGE_CALLS}
    assert rounds[2048, 8] == 8 and rounds[2048, 9] == 8 and rounds[17, 964] == 963 and rounds[2047, 1024] == 8
    assert 964 % 4 == 0 and 9 % 2 == 1 and 9 % 4 == 1                              # whole and ragged last groups
    for M, Ds, K in SHAPES:                                                        # which build loop a shape takes
        assert (Ds % 4 == 0) == ((M, Ds, K) in SHAPES[:3])
    assert 12 // 4 == 3 and 200 < 256                                              # three dwordx4 steps and the +inf tail
    cap = lambda k: 2 * max(256, 1 << (k - 1).bit_length())
    assert sorted({cap(k) for k in KS}) == [512, 1024, 2048, 4096]
    assert all(LONG > cap(k) for k in KS) and all(EQUAL > cap(k) for k in KS if k <= 512)  # a refresh at every cap


@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
def test_the_refresh_case_is_what_it_is_built_to_be(plain):
    c = refresh_case(plain)
    assert np.diff(c["offsets"]).tolist() == [LONG, EQUAL, 50, 30, 120, 0, 0]
    long_ids, equal_ids = c["ids"][:LONG], c["ids"][LONG:LONG + EQUAL]
    d = [RR.list_keys(c, q, 0) >> np.uint64(32) for q in c["qs"]]
    assert np.all(np.diff(d[0].astype(np.int64)) < 0) and np.all(np.diff(d[1].astype(np.int64)) > 0)  # strictly
    assert len(np.unique(RR.list_keys(c, c["qs"][0], 1) >> np.uint64(32))) == 1    # every distance of list 1 equal
    for k in KS:
        alone = c["alone"][0][k]
        assert np.array_equal(alone[0][0], long_ids[::-1][:k]) and np.array_equal(alone[0][1], long_ids[:k])
        assert np.array_equal(c["alone"][1][k][0][0, :min(k, EQUAL)], equal_ids[:k])   # the k lowest ids
        assert np.all(c["alone"][1][k][0][0, EQUAL:] == -1)
        far = c["alone"][2][k]
        assert far[1][0][0] > alone[1][0][k - 1]                                   # list 2 starts above list 0's last threshold
        assert (far[0][0] >= 0).sum() == 50 and np.isposinf(far[1][0][50])         # and its rows appear when probed alone
        assert np.array_equal(c["want"][k][0][0], alone[0][0])                     # ... and not behind list 0


# ---- 1. wide and scalar sub-spaces --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sub_spaces_of_every_width(gpu, monkeypatch, shape, plain):
    """Ds = 8 and 12: two and three dwordx4 steps per sub-space, at M = 8 and 16; K = 200 with Ds = 12 the +inf tail beside
    them; Ds = 1 (M = 16: D = 16) and K = 7 the scalar path at its smallest.  Lists of 0, 1, 255, 256, 257, 600 and the
    rest; nprobe = 5; host and device forms."""
    import torch
    c = T.make_case(*shape, plain)
    assert np.diff(c["offsets"]).tolist()[:6] == list(T.LENGTHS)
    want = RR.search_at(c, c["qs"], T.PROBES, (1, 100))
    idx, ivf = T.open_case(gpu, c)
    with idx, ivf:
        for P in (1, 2, 4):
            T.with_group(monkeypatch, P)
            for k in (1, 100):
                assert RR.same(ivf.search_probes_residual(c["qs"], T.PROBES, k), want[k]), (shape, plain, k, P)
        t_q, t_p = device(torch, c["qs"], T.PROBES)
        assert RR.same(host(ivf.search_probes_residual_torch(t_q, t_p, 100)), want[100]), (shape, plain, "device form")


# ---- 2. top_k and the refresh at every cap -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
def test_top_k_and_the_refresh_at_every_buffer_size(gpu, monkeypatch, plain):
    """cap = 512, 1024, 2048 and 4096: the sort at each size, the refresh `cnt + 256 > cap`, the threshold at a top_k that
    is no power of two, the emit loop beyond its first pass.  Query 0 lowers the threshold with every refresh, query 1
    never appends after the first, list 1 is decided by ids alone, and the far lists 2 and 3 follow in the same group."""
    c = refresh_case(plain)
    idx, ivf = T.open_case(gpu, c)
    with idx, ivf:
        for P in (4, 2):
            T.with_group(monkeypatch, P)
            for k in KS:
                assert RR.same(ivf.search_probes_residual(c["qs"], c["probes"], k), c["want"][k]), (plain, P, k)
        for l in (0, 1, 2):
            for k in KS:
                assert RR.same(ivf.search_probes_residual(c["qs"], [[l], [l]], k), c["alone"][l][k]), (plain, "list", l, k)


# ---- 3. the device forms ---------------------------------------------------------------------------------------------------

def allowed_of(c, n_ids, empty_list):
    """About 10 % of the ids, none of them in `empty_list`, the last id (the renamed node of an even DTC index) among them."""
    allowed = np.random.default_rng(3).random(n_ids) < 0.1
    allowed[n_ids - 1] = True
    allowed[c["ids"][c["offsets"][empty_list]:c["offsets"][empty_list + 1]]] = False
    return allowed


def device_forms(api, c, idx, ivf, probes, k, nprobe, empty_list, what):
    import torch
    qs = c["qs"][:len(probes)]
    t_q, t_p = device(torch, qs, probes)
    allowed = allowed_of(c, c["n"] + 1, empty_list)
    with api.IdFilter.from_mask(idx, allowed) as f:
        for filt, mask in ((None, None), (f, allowed)):
            want = RR.search(c, qs, probes, k, mask)
            assert RR.same(ivf.search_probes_residual(qs, probes, k, id_filter=filt), want), what
            assert RR.same(host(ivf.search_probes_residual_torch(t_q, t_p, k, id_filter=filt)), want), what
            out = torch.full((len(qs), k), 7, dtype=torch.int32).cuda(), torch.full((len(qs), k), 7.0).cuda()
            got = ivf.search_probes_residual_torch(t_q, t_p, k, out_ids=out[0], out_dists=out[1], id_filter=filt)
            assert got[0] is out[0] and got[1] is out[1] and RR.same(host(out), want), what + ": the caller's outputs"
            lists, _ = ivf.probe(qs, nprobe)
            want = RR.search(c, qs, lists, k, mask)
            assert RR.same(ivf.search_residual(qs, nprobe, k, id_filter=filt), want), what
            out = torch.full((len(qs), k), 7, dtype=torch.int32).cuda(), torch.full((len(qs), k), 7.0).cuda()
            ivf.search_residual_torch(t_q, nprobe, k, out_ids=out[0], out_dists=out[1], id_filter=filt)
            assert RR.same(host(out), want) and RR.same(host(ivf.search_residual_torch(t_q, nprobe, k, id_filter=filt)), want), what
        only = ivf.search_probes_residual_torch(t_q, device(torch, np.full((len(qs), 1), empty_list, dtype=np.int32))[0], 10, id_filter=f)
        assert np.all(host(only)[0] == -1) and np.all(np.isposinf(host(only)[1])), what + ": nothing allowed in the list"


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
@pytest.mark.parametrize("shape", SHAPES + ["refresh"], ids=str)
def test_the_device_forms_answer_as_the_host_forms_do(gpu, shape, plain):
    """search_probes_residual_torch and search_residual_torch, with and without an IdFilter (about 10 % allowed, nothing in
    one list), into their own and into the caller's outputs."""
    if shape == "refresh":
        c = refresh_case(plain)
        probes, k, empty = c["probes"], 1025, 2
    else:
        c = T.make_case(*shape, plain)
        probes, k, empty = T.PROBES, 100, 5
    idx, ivf = T.open_case(gpu, c)
    with idx, ivf:
        device_forms(gpu, c, idx, ivf, probes, k, 3, empty, "%s %s" % (shape, "plain" if plain else "dtc"))


# ---- 4. slices and rounds ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
def test_two_slices_of_queries(gpu, plain):
    """nq = 2049 at nprobe 2, top_k 3, nlist 7: a slice of 2048 queries and one of 1, whose queries start at q0 = 2048."""
    c = T.make_case(8, 4, 256, plain)
    nq, k = 2049, 3
    probes = np.random.default_rng(31).integers(-1, T.NLIST, size=(nq, 2)).astype(np.int32)
    probes[-1] = [4, 6]
    use = np.arange(nq) % T.NQ
    use[-1] = 3
    qs = np.ascontiguousarray(c["qs"][use])
    want = RR.search_at(c, c["qs"], probes, (k,), use=use)[k]
    last = RR.search(c, c["qs"][3:4], [[4, 6]], k)
    assert RR.same((want[0][-1:], want[1][-1:]), last) and np.all(last[0] >= 0)
    idx, ivf = T.open_case(gpu, c)
    with idx, ivf:
        got = ivf.search_probes_residual(qs, probes, k)
        assert RR.same((got[0][-1:], got[1][-1:]), last), "the last query, alone in its slice"
        assert RR.same(got, want)
        refused_in_the_last_row(gpu, ivf, qs, probes, T.NLIST, k, want, "nq 2049")
        assert RR.same(ivf.search_probes_residual(qs, probes, k), want), "the host form after the refused call"


@pytest.mark.gpu
@pytest.mark.parametrize("top_k,nprobe", MERGE_CALLS)
def test_merge_rounds_and_ragged_groups(gpu, monkeypatch, top_k, nprobe):
    """1024 lists: nprobe = round and round + 1 at top_k 2048, a round of 963 lists under 964 probes, 147 rounds at (2047,
    1024); a grid of up to 512 groups whose last one is ragged wherever P does not divide nprobe."""
    c = lists_case()
    nq = 5
    probes = prefixes(nq, c["nlist"], nprobe, 40 + nprobe)
    want = RR.search_at(c, c["qs"], probes, (top_k,), use=np.arange(nq), memo=c["memo"])[top_k]
    idx, ivf = open_lists(gpu, c)
    with idx, ivf:
        for P in (2, 4):
            T.with_group(monkeypatch, P)
            assert RR.same(ivf.search_probes_residual(c["qs"], probes, top_k), want), (top_k, nprobe, P)
        refused_in_the_last_row(gpu, ivf, c["qs"], probes, c["nlist"], top_k, want, "top-%d of %d lists" % (top_k, nprobe))


@pytest.mark.gpu
def test_slices_of_sixteen_queries(gpu):
    """nq = 33 at nprobe 1024, top_k 2048: slices of 16, 16 and 1 query, each merged in rounds of 8 lists."""
    c = lists_case()
    nq, k = 33, 2048
    probes = prefixes(nq, c["nlist"], 1024, 51)
    use = np.arange(nq) % 5
    use[-1] = 2
    qs = np.ascontiguousarray(c["qs"][use])
    want = RR.search_at(c, c["qs"], probes, (k,), use=use, memo=c["memo"])[k]
    assert np.all(want[0] >= 0) and not RR.same((want[0][:1], want[1][:1]), (want[0][16:17], want[1][16:17]))
    idx, ivf = open_lists(gpu, c)
    with idx, ivf:
        assert RR.same(ivf.search_probes_residual(qs, probes, k), want)
        refused_in_the_last_row(gpu, ivf, qs, probes, c["nlist"], k, want, "33 queries, 1024 lists")
