"""IVF search over raw vectors (dpq_flat_ivf_*) where its first suite (tests/test_ivf_flat.py) stops: every group at widths
of several slices and at the widest rows, the key sink cut at every buffer size with unequal counts in one stretch, fp32
overflow and denormal distances, the list build and the pair sort from 1 to 65536 lists, calls cut into slices of sixteen
queries, buffers that grow, device queries off their alignment.

Every comparison is strict -- ids equal, distances equal as fp32 bit patterns, padding -1 / +inf -- against
tests/_flat_ivf_restatement.py.  Nothing is skipped and no case is exempt.

Choices the issue leaves open, and why:
 * the wide cases (D = 2045, 2048) keep lists of 0, 1, 255, 256, 257 and 40 rows, 846 rows in all; their probe matrix is the
   first suite's with its lists renamed: 17, 16, 15, 1 and 1 queries on lists 4, 3, 2, 1 and 0, the short list, -1 and
   repeats.
 * the sink case: the rows of the long list are (i / 4, 0, 0, 0) in list order.  Queries 0 .. 6 lie beyond its far end (the
   nearest rows come last: every tile is appended whole), queries 7 .. 14 before its near end (nothing is appended behind
   the first cut), so the counts of one stretch differ at every cut; query 15 is (2^40, 0, 0, 0), whose fp32 difference to
   every row of the list is -2^40: all 4500 distances are 2^80 and the id decides.  A fifth list holds 5000 rows in no
   order, and four more are in nearest-first order for queries 7 .. 14 but for the row that is their 255th (511th, 1023rd,
   2047th) nearest, which comes last: behind the cuts a single row arrives whose key lies between the k-th and the k - 1-th
   of the buffer.  Every pair of a stretch scans the same
   rows under the threshold kFlatNoKey until the first cut, so no count is below top_k when a cut happens: that branch of
   sink_make_room cannot be reached without a filter, and is not claimed here.
"""
import numpy as np
import pytest

import _flat_ivf_restatement as FR
import test_ivf_flat as T

F32 = np.float32
KS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
WIDE_LENGTHS = (0, 1, 255, 256, 257, 40)
LONG, EQUAL, MIXED = 4500, 1500, 5000
LATE = {255: 600, 511: 1100, 1023: 2200, 2047: 4200}   # top_k: rows of the list whose top_k-th nearest row comes last
ALONE = (0, 1, 2, 4, 5, 6, 7, 8)
_cache = {}


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def with_group(monkeypatch, G):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))


def device(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def host(got):
    return got[0].cpu().numpy(), got[1].cpu().numpy()


def labelled(lengths, extra, seed):
    """(labels, offsets, rows): row 0 and `extra` - 1 more rows in no list, the rest dealt to lists of the given lengths."""
    rng = np.random.default_rng(seed)
    n = sum(lengths) + extra
    labels = np.full(n, -1, dtype=np.int32)
    labels[1 + rng.permutation(n - 1)[:sum(lengths)]] = np.repeat(np.arange(len(lengths)), lengths)
    return (labels,) + FR.lists_from_labels(labels, len(lengths))


def wide_case(D):
    """Lists of WIDE_LENGTHS over 846 rows of D dimensions; the wanted top-100 of its probe matrix, made once."""
    if ("wide", D) in _cache:
        return _cache["wide", D]
    rng = np.random.default_rng(D)
    labels, offsets, rows = labelled(WIDE_LENGTHS, 37, D)
    base = rng.standard_normal((len(labels), D)).astype(F32)
    of4 = rows[offsets[4]:offsets[5]]
    base[of4[1::2]] = base[of4[0:-1:2]]                                            # equal distances: the id decides
    q = np.arange(T.NQ)
    col0 = np.select([q < 17, q < 33, q < 48, q < 49], [4, 3, 2, 1], 0)            # 17, 16, 15, 1 and 1 queries per list
    probes = np.stack([col0, np.full(T.NQ, 5), np.where(q % 2 == 0, -1, 2 + q % 3), np.where(q % 5 == 0, col0, q % 2 * 5)], 1)
    c = dict(D=D, base=base, labels=labels, offsets=offsets, rows=rows, probes=probes.astype(np.int32), nlist=len(WIDE_LENGTHS),
             qs=(F32(0.1) * rng.standard_normal((T.NQ, D))).astype(F32))
    c["want"] = FR.search(c, c["qs"], c["probes"], 100)
    _cache["wide", D] = c
    return c


def narrow_case(D):
    """The first suite's case at D, with the wanted top-100 of its probe matrix made once."""
    if ("narrow", D) not in _cache:
        c = T.make_case(D)
        _cache["narrow", D] = dict(c, nlist=T.NLIST, want=FR.search(c, c["qs"], c["probes"], 100))
    return _cache["narrow", D]


def sink_case():
    if "sink" in _cache:
        return _cache["sink"]
    rng = np.random.default_rng(61)
    labels, offsets, rows = labelled((LONG, EQUAL, 50, 30, MIXED) + tuple(LATE.values()), 37, 62)
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    base = rng.standard_normal((len(labels), 4)).astype(F32)                       # (list 4 stays as drawn)
    base[of(0)] = 0
    base[of(0), 0] = np.arange(LONG) / 4
    base[of(1)] = [3.5, -2.25, 1.0, 0.5]
    base[of(2)] += F32(3000)
    base[of(3)] += F32(3000)
    for l, (k, length) in enumerate(LATE.items(), 5):                              # nearest first, but for the k-th nearest
        order = np.concatenate([np.arange(k - 1), np.arange(k, length), [k - 1]])
        base[of(l)] = 0
        base[of(l), 0] = order / 4
    qs = np.zeros((16, 4), dtype=F32)
    qs[:7, 0] = (LONG - 1) / 4 + 0.5 + np.arange(7)                                # beyond the far end: nearest last
    qs[7:15, 0] = -0.5 - np.arange(8)                                              # before the near end: nearest first
    qs[15, 0] = 2.0 ** 40
    c = dict(base=base, labels=labels, offsets=offsets, rows=rows, qs=qs, nlist=9,
             probes=np.tile(np.arange(9, dtype=np.int32), (16, 1)))
    c["want"] = FR.search_at(c, qs, c["probes"], KS)
    c["alone"] = {l: FR.search_at(c, qs, np.full((16, 1), l, dtype=np.int32), KS) for l in ALONE}
    _cache["sink"] = c
    return c


def open_flat(api, c, id_offset=0, labels=None):
    flat = api.FlatIndex(c["base"], id_offset=id_offset)
    return flat, api.FlatIVF.from_labels(flat, c["labels"] if labels is None else labels, c["nlist"])


# ---- CPU: what the shapes below rest on --------------------------------------------------------------------------------------

TILE_BYTES = 32 * 260 * 4 + 32 * 16 * 4 + 256 * 4                                  # rows, queries, row numbers of a tile


def cap_of(top_k):
    return 2 * max(256, 1 << (top_k - 1).bit_length())


def group_of(top_k, group):
    """dpq_flat_ivf.hip's flat_ivf_group: the largest of 16 .. 1 that is at most `group` and fits 160 KB of LDS."""
    g = 16
    while g > 1 and (g > group or TILE_BYTES + g * cap_of(top_k) * 8 + 512 > 160 * 1024):
        g >>= 1
    return g


def slices_of(nq, nprobe, top_k):
    return max(1, min(nq, 2048, (256 << 20) // (nprobe * top_k * 8))), 16384 // top_k


def key_bits(nlist):
    bits = 1
    while (1 << bits) <= nlist:
        bits += 1
    return bits


def test_the_shapes_cross_the_edges_they_are_chosen_for():
    assert [group_of(100, G) for G in (1, 2, 4, 8, 16)] == [1, 2, 4, 8, 16]         # top-100: every group is what was asked
    assert [-(-D // 4) * 4 for D in (100, 36, 2045, 2048)] == [100, 36, 2048, 2048]
    assert [min(32, 100 - d) for d in range(0, 100, 32)] == [32, 32, 32, 4] and 36 - 32 == 4
    assert sorted({cap_of(k) for k in KS}) == [512, 1024, 2048, 4096]
    assert LONG > 4096 - 256 and EQUAL > 1024 - 256                                 # a cut at every cap; equal rows across two
    assert [group_of(k, 16) for k in (255, 257, 513, 1025)] == [16, 8, 4, 2]        # the sixteen queries: one stretch at cap 512
    assert slices_of(33, 1024, 2048) == (16, 8) and 33 - 2 * 16 == 1
    assert [key_bits(n) for n in (1, 2, 256, 4096, 65536)] == [1, 2, 9, 13, 17]     # the padding key nlist needs one bit more
    assert [key_bits(n - 1) for n in (2, 256, 4096, 65536)] == [1, 8, 12, 16]


def test_the_sink_case_is_what_it_is_built_to_be():
    c = sink_case()
    long_rows, equal_rows = c["rows"][:LONG], c["rows"][LONG:LONG + EQUAL]
    for k in KS:
        ids, dists = c["alone"][0][k]
        for q in range(7):
            assert np.array_equal(ids[q], long_rows[::-1][:k]) and np.all(np.diff(dists[q]) > 0)   # the last k rows
        for q in range(7, 15):
            assert np.array_equal(ids[q], long_rows[:k]) and np.all(np.diff(dists[q]) > 0)
        assert np.array_equal(ids[15], long_rows[:k]) and np.all(dists[15] == F32(2.0 ** 80))       # equidistant: by id
        assert np.array_equal(c["alone"][1][k][0][3, :min(k, EQUAL)], equal_rows[:k])               # the k lowest ids
        assert len(np.unique(c["alone"][1][k][1][3, :min(k, EQUAL)])) == 1
        far = c["alone"][2][k]
        assert far[1][0][0] > dists[0][k - 1] and (far[0][0] >= 0).sum() == 50     # above list 0's last threshold; alone: all there
        mixed, at = c["alone"][4][k][0][0], {r: i for i, r in enumerate(c["rows"][LONG + EQUAL + 80:])}
        assert sum(at.get(r, 0) >= cap_of(k) for r in mixed) > k // 8              # rows of the answer that arrive behind a cut
    for l, (k, length) in enumerate(LATE.items(), 5):
        late = c["rows"][c["offsets"][l]:c["offsets"][l + 1]]
        ids = c["alone"][l][k][0][7]
        assert length > cap_of(k) and ids[k - 1] == late[-1] and np.array_equal(ids[:k - 1], late[:k - 1])  # the k-th comes last


def overflow_case():
    """List 0: 300 rows about 1e20 from the query in every dimension.  List 1: 300 rows 2^-70 * j from it, j = 1 .. 60."""
    rng = np.random.default_rng(71)
    labels = np.repeat(np.array([0, 1, -1], dtype=np.int32), [300, 300, 5])[rng.permutation(605)]
    offsets, rows = FR.lists_from_labels(labels, 2)
    q = (2.0 ** -60 * np.array([[1, 2, 3, 4]])).astype(F32)
    base = np.zeros((605, 4), dtype=F32)
    base[rows[:300]] = (F32(1e20) * (1 + rng.random((300, 4)))).astype(F32) * rng.choice([-1, 1], (300, 4)).astype(F32)
    base[rows[300:]] = q + (2.0 ** -70 * rng.integers(1, 61, (300, 4))).astype(F32)
    return dict(base=base, labels=labels, offsets=offsets, rows=rows, qs=q, nlist=2)


def test_the_numeric_case_is_what_it_is_built_to_be():
    c = overflow_case()
    with np.errstate(over="ignore"):
        ids, dists = FR.search(c, c["qs"], [[0]], 400)
    assert np.array_equal(ids[0, :300], c["rows"][:300]) and np.all(np.isposinf(dists)) and np.all(ids[0, 300:] == -1)
    ids, dists = FR.search(c, c["qs"], [[1]], 400)
    d = dists[0, :300]
    assert np.all(d > 0) and np.all(d < F32(2.0 ** -126)) and len(np.unique(d)) >= 16 and np.all(ids[0, :300] >= 0)
    exact = ((c["base"][ids[0, :300]].astype(np.float64) - c["qs"][0].astype(np.float64)) ** 2).sum(axis=1)
    assert np.array_equal(d.astype(np.float64), exact)                              # every square and sum is exact


# ---- 5. groups x slices ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("D", [100, 36, 2045, 2048])
def test_every_group_at_every_width(gpu, monkeypatch, D, G):
    """D = 100: slices of 32, 32, 32 and 4 dimensions; 36: one and a short one; 2045: rows padded to 2048; 2048: the widest.
    G = 8 is the QPL = 2 kernel, G = 16 the QPL = 4 one."""
    with_group(monkeypatch, G)
    c = wide_case(D) if D > 2000 else narrow_case(D)
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        assert FR.same(ivf.search_probes(c["qs"], c["probes"], 100), c["want"]), (D, G)


# ---- 6. the sink at every cap ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("G", [16, 4, None], ids=["G16", "G4", "shipped"])
def test_the_sink_is_cut_at_every_buffer_size(gpu, monkeypatch, G):
    """Sixteen queries on one list of 4500 rows: at G = 16 and top_k <= 256 one stretch of sixteen pairs, beyond that the
    stretches the LDS leaves (8, 4, 2); cuts at cap 512, 1024, 2048 and 4096 with the counts of a stretch apart; 1500 equal
    rows across the cuts of caps 512 and 1024."""
    if G is not None:
        with_group(monkeypatch, G)
    c = sink_case()
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        for k in KS:
            assert FR.same(ivf.search_probes(c["qs"], c["probes"], k), c["want"][k]), (G, k)
        for l in ALONE:
            for k in KS:
                assert FR.same(ivf.search_probes(c["qs"], np.full((16, 1), l, dtype=np.int32), k), c["alone"][l][k]), (G, l, k)


# ---- 7. numeric edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_overflow_and_denormal_distances(gpu):
    """+inf distances keep their ids, in id order, ahead of the padding; denormal squares and sums are not flushed."""
    c = overflow_case()
    with np.errstate(over="ignore"):
        want = {p: FR.search(c, c["qs"], [p], 400) for p in ((0,), (1,), (0, 1), (1, 0))}
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        for p in want:
            assert FR.same(ivf.search_probes(c["qs"], [list(p)], 400), want[p]), p


# ---- 8. nlist and the pair sort ----------------------------------------------------------------------------------------------------

def check_structure(ivf, c, id_offset, what):
    got = ivf.lists()
    assert np.array_equal(got[0], c["offsets"]) and np.array_equal(got[1], c["rows"] + id_offset), what
    inf = ivf.info()
    want = (c["nlist"], (c["labels"] >= 0).sum(), (c["labels"] < 0).sum(), np.diff(c["offsets"]).max())
    assert (inf["nlist"], inf["n_assigned"], inf["n_unassigned"], inf["max_list_len"]) == want, "%s: %s" % (what, inf)


def small_case(nlist, labels=None):
    n = 3000
    rng = np.random.default_rng(81)
    base = rng.standard_normal((n, 4)).astype(F32)
    if labels is None:
        labels = rng.integers(0, nlist, size=n).astype(np.int32)
        labels[rng.random(n) < 0.10] = -1
        labels[[5, n - 1]] = nlist - 1
    c = dict(base=base, labels=labels, nlist=nlist, qs=rng.standard_normal((5, 4)).astype(F32))
    c["offsets"], c["rows"] = FR.lists_from_labels(labels, nlist)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("nlist", [1, 2, 256, 4096, 65536])
def test_from_one_list_to_65536(gpu, nlist):
    """The list build and the pair sort at key widths of 1, 2, 9, 13 and 17 bits; host and device labels; ids that end at
    2^31 - 1."""
    import torch
    c = small_case(nlist)
    n, off = len(c["labels"]), 2 ** 31 - 1 - 3000
    assert (c["labels"] < 0).sum() > 200 and c["labels"].max() == nlist - 1
    nprobe = min(nlist, 1024)
    rng = np.random.default_rng(82)
    probes = np.stack([np.concatenate([[nlist - 1], rng.permutation(nlist - 1)[:nprobe - 1]]) for _ in range(5)]).astype(np.int32)
    want = FR.search(c, c["qs"], probes, 300, id_offset=off)
    assert off + n - 1 == 2 ** 31 - 2 and n - 1 in c["rows"][c["offsets"][nlist - 1]:]  # the largest id is in the first list probed
    assert np.all(want[0][want[0] != -1] >= off)                                    # no id wraps
    for name, lab in (("host labels", c["labels"]), ("device labels", torch.from_numpy(c["labels"]).cuda())):
        flat, ivf = open_flat(gpu, c, id_offset=off, labels=lab)
        with flat, ivf:
            check_structure(ivf, c, off, "nlist %d, %s" % (nlist, name))
            assert FR.same(ivf.search_probes(c["qs"], probes, 300), want), (nlist, name)


@pytest.mark.gpu
def test_every_row_in_the_last_list_and_none_in_any(gpu):
    n, nlist = 3000, 65536
    probes = np.tile(np.array([17, 65535, -1, 0], dtype=np.int32), (5, 1))
    c = small_case(nlist, np.full(n, nlist - 1, dtype=np.int32))
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        check_structure(ivf, c, 0, "every row in list 65535")
        assert c["offsets"][nlist - 1] == 0 and np.array_equal(c["rows"], np.arange(n))
        for k in (10, 2048):
            got = ivf.search_probes(c["qs"], probes, k)
            assert FR.same(got, FR.search(c, c["qs"], probes, k)) and FR.same(got, flat.search(c["qs"], k)), k
    c = small_case(nlist, np.full(n, -1, dtype=np.int32))
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        check_structure(ivf, c, 0, "every row unassigned")
        got = ivf.search_probes(c["qs"], probes, 10)
        assert np.all(got[0] == -1) and np.all(np.isposinf(got[1])), "every search is all padding"


# ---- 9. slices, growth, alignment ------------------------------------------------------------------------------------------------

def lists_case():
    if "lists" in _cache:
        return _cache["lists"]
    n, nlist = 6000, 1024
    rng = np.random.default_rng(91)
    c = dict(base=rng.standard_normal((n, 4)).astype(F32), labels=rng.integers(0, nlist, size=n).astype(np.int32), nlist=nlist,
             qs=rng.standard_normal((33, 4)).astype(F32))
    c["offsets"], c["rows"] = FR.lists_from_labels(c["labels"], nlist)
    _cache["lists"] = c
    return c


def prefixes(nq, nlist, nprobe, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int32)


@pytest.mark.gpu
def test_slices_of_sixteen_queries(gpu):
    """nq = 33 at nlist = nprobe = 1024, top_k 2048: slices of 16, 16 and 1 query; every row is labelled and every list
    probed, so the answer is the exact search's."""
    c = lists_case()
    probes = prefixes(33, 1024, 1024, 92)
    want = FR.search(c, c["qs"], probes, 2048)
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        got = ivf.search_probes(c["qs"], probes, 2048)
        assert FR.same(got, want) and FR.same(got, flat.search(c["qs"], 2048))


@pytest.mark.gpu
def test_a_call_that_grows_every_buffer(gpu):
    """On one fresh structure: top-10 of 2 lists, then top-2048 of 1024 (every buffer grows, the rounds' own appear), then
    top-10 again in the grown buffers."""
    c = lists_case()
    qs = c["qs"][:5]
    small, every = prefixes(5, 1024, 2, 93), prefixes(5, 1024, 1024, 94)
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        assert FR.same(ivf.search_probes(qs, small, 10), FR.search(c, qs, small, 10))
        got = ivf.search_probes(qs, every, 2048)
        assert FR.same(got, FR.search(c, qs, every, 2048)) and FR.same(got, flat.search(qs, 2048))
        assert FR.same(ivf.search_probes(qs, small, 10), FR.search(c, qs, small, 10))


@pytest.mark.gpu
def test_device_queries_off_their_alignment(gpu):
    """D = 32 = Dp: aligned device queries are read where they are; one float further on they are copied first."""
    import torch
    c = narrow_case(32)
    t_p = device(torch, c["probes"])[0]
    buf = torch.zeros(T.NQ * 32 + 8, dtype=torch.float32).cuda()
    buf[1:1 + T.NQ * 32] = torch.from_numpy(c["qs"].ravel()).cuda()
    moved = buf[1:1 + T.NQ * 32].view(T.NQ, 32)
    aligned = device(torch, c["qs"])[0]
    assert moved.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and moved.is_contiguous()
    flat, ivf = open_flat(gpu, c)
    with flat, ivf:
        assert FR.same(host(ivf.search_probes_torch(aligned, t_p, 100)), c["want"])
        assert FR.same(host(ivf.search_probes_torch(moved, t_p, 100)), c["want"])
