"""IVF search over byte vectors (dpq_flat_ivf_*_bytes) where its first suite (tests/test_ivf_flat_bytes.py) stops: wide rows
in lists that fill MFMA blocks, wavefronts and tiles, a half K step in the middle of the widths, the groups the LDS leaves
beside wide rows and a large top_k, the key sink cut at every buffer size, calls cut into query slices, the coarse step
across a slice boundary, device queries off their alignment.

Every comparison is strict -- ids equal, distances equal as fp32 bit patterns, padding -1 / +inf -- against
tests/_flat_ivf_restatement.py, which is exact in int64.  Nothing is skipped and no case is exempt.

Choices the issue leaves open, and why:
 * the wide cases keep lists of 0, 1, 15, 16, 17, 63, 64, 65, 255, 256 and 257 rows; their probe matrix is the first suite's
   with its lists renamed: 17, 16, 15, 1 and 1 queries on lists 10, 9, 8, 7 and 1, then lists 1 .. 8 in turn, -1 and repeats.
 * the sink case: row i of the long list is (i // 18, 0, 0) + 2 in list order, 250 runs of 18 equal rows on a line.  Queries
   0 .. 7 are (255, 2, 2) (the nearest rows come last), queries 8 .. 15 (0, 2, 2) (nearest first), each with another
   second byte, so the counts of one stretch differ at every cut.  Bytes on a line cannot be equidistant from a query
   unless they are equal: the list of 1500 equal rows is that case.  A fifth list holds 5000 rows in no order, and four more
   are in nearest-first order for queries 8 .. 15 but for the row that is their 255th (511th, 1023rd, 2047th) nearest, which
   comes last: behind the cuts a single row arrives whose key lies between the k-th and the k - 1-th of the buffer.
"""
import numpy as np
import pytest

import _flat_ivf_restatement as FR
import test_ivf_flat_bytes as T

F32 = np.float32
KINDS = T.KINDS
KS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
WIDE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
LONG, EQUAL, MIXED = 4500, 1500, 5000
# top_k: (rows, run) of the list whose top_k-th nearest row comes last; rows lie in runs of `run` equal ones
LATE = {255: (600, 127), 511: (1100, 10), 1023: (2200, 73), 2047: (4200, 62)}
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


def as_kind(kind, a):
    """Values 0 .. 255 as the kind's bytes: lowered by 128 for int8."""
    dtype, lower = KINDS[kind]
    return (np.asarray(a) - lower).astype(dtype)


def labelled(lengths, extra, seed):
    """(labels, offsets, rows): row 0 and `extra` - 1 more rows in no list, the rest dealt to lists of the given lengths."""
    rng = np.random.default_rng(seed)
    n = sum(lengths) + extra
    labels = np.full(n, -1, dtype=np.int32)
    labels[1 + rng.permutation(n - 1)[:sum(lengths)]] = np.repeat(np.arange(len(lengths)), lengths)
    return (labels,) + FR.lists_from_labels(labels, len(lengths))


def open_bytes(api, c, centroids=None):
    flat = (api.FlatIndexU8 if c["kind"] == "u8" else api.FlatIndexI8)(c["base"])
    return flat, api.FlatIVFBytes.from_labels(flat, c["labels"], c["nlist"], centroids=centroids)


def wide_case(kind, D):
    if ("wide", kind, D) in _cache:
        return _cache["wide", kind, D]
    rng = np.random.default_rng(D)
    labels, offsets, rows = labelled(WIDE_LENGTHS, 37, D)
    base = rng.integers(0, 256, (len(labels), D))
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    base[of(9)[100:104]], base[of(9)[200:204]] = 0, 255                             # the extreme rows inside a full tile
    base[of(7)[10:14]] = 255                                                        # ... and where query 48 reports every row
    base[of(10)[1::2]] = base[of(10)[0:-1:2]]                                       # equal distances: the id decides
    q = np.arange(T.NQ)
    col0 = np.select([q < 17, q < 33, q < 48, q < 49], [10, 9, 8, 7], 1)            # 17, 16, 15, 1 and 1 queries per list
    probes = np.stack([col0, 1 + q % 8, np.where(q % 2 == 0, -1, 4 + q % 3), np.where(q % 5 == 0, col0, q % 2 * 7)], 1)
    qs = rng.integers(0, 256, (T.NQ, D))
    qs[0], qs[17], qs[48] = 255, 0, 0                                               # the largest distances: D * 255^2
    c = dict(kind=kind, D=D, base=as_kind(kind, base), labels=labels, offsets=offsets, rows=rows, nlist=len(WIDE_LENGTHS),
             probes=probes.astype(np.int32), qs=as_kind(kind, qs))
    c["want"] = FR.search(c, c["qs"], c["probes"], 100)
    _cache["wide", kind, D] = c
    return c


def lds_case(kind, D):
    """Ten lists, one of 300 rows; twenty queries that probe nine of them."""
    if ("lds", kind, D) in _cache:
        return _cache["lds", kind, D]
    rng = np.random.default_rng(D + 1)
    labels, offsets, rows = labelled((300, 40, 17, 0, 1, 64, 65, 30, 16, 20), 7, D + 1)
    c = dict(kind=kind, D=D, base=as_kind(kind, rng.integers(0, 256, (len(labels), D))), labels=labels, offsets=offsets, rows=rows,
             nlist=10, qs=as_kind(kind, rng.integers(0, 256, (20, D))),
             probes=np.stack([(q + np.arange(9)) % 10 for q in range(20)]).astype(np.int32))
    c["want"] = FR.search_at(c, c["qs"], c["probes"], (1025, 2048))
    _cache["lds", kind, D] = c
    return c


def sink_case(kind):
    if ("sink", kind) in _cache:
        return _cache["sink", kind]
    rng = np.random.default_rng(61)
    labels, offsets, rows = labelled((LONG, EQUAL, 50, 30, MIXED) + tuple(n for n, _ in LATE.values()), 37, 62)
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    base = rng.integers(0, 256, (len(labels), 3))                                   # (list 4 stays as drawn: rows in no order)
    base[of(0)] = 2
    base[of(0), 0] += np.arange(LONG) // 18
    base[of(1)] = [40, 7, 200]
    base[of(2), 1:] = 255 - base[of(2), 1:] % 8                                     # far: about 2 * 250^2 from every query
    base[of(3), 1:] = 255 - base[of(3), 1:] % 8
    for l, (k, (length, run)) in enumerate(LATE.items(), 5):                        # nearest first in runs of even values; the
        assert (k - 1) % run == 0 and 2 * (length // run) < 250                     # last row, an odd value, is the k-th nearest
        base[of(l)] = 2
        base[of(l), 0] = 2 * (np.arange(length) // run)
        base[of(l)[-1], 0] = 2 * ((k - 1) // run) - 1
    qs = np.full((16, 3), 2)
    qs[:8, 0], qs[8:, 0], qs[:, 1] = 255, 0, 2 + np.arange(16) % 8
    c = dict(kind=kind, base=as_kind(kind, base), labels=labels, offsets=offsets, rows=rows, qs=as_kind(kind, qs), nlist=9,
             probes=np.tile(np.arange(9, dtype=np.int32), (16, 1)))
    c["want"] = FR.search_at(c, c["qs"], c["probes"], KS)
    c["alone"] = {l: FR.search_at(c, c["qs"], np.full((16, 1), l, dtype=np.int32), KS) for l in ALONE}
    _cache["sink", kind] = c
    return c


# ---- CPU: what the shapes below rest on --------------------------------------------------------------------------------------

def cap_of(top_k):
    return 2 * max(256, 1 << (top_k - 1).bit_length())


def tile_bytes(Dp):
    """dpq_flat_ivf_u8.hip: sixteen staged queries of Dp + 16 bytes, and the row numbers of a tile."""
    return 16 * (Dp + 16) + 256 * 4


def group_u8(top_k, Dp, group):
    """dpq_flat_ivf_u8.hip's flat_ivf_group_u8: the largest of 16 .. 1 that is at most `group` and fits 160 KB of LDS."""
    g = 16
    while g > 1 and (g > group or tile_bytes(Dp) + g * cap_of(top_k) * 8 + 512 > 160 * 1024):
        g >>= 1
    return g


def slices_of(nq, nprobe, top_k):
    return max(1, min(nq, 2048, (256 << 20) // (nprobe * top_k * 8))), 16384 // top_k


def test_the_shapes_cross_the_edges_they_are_chosen_for():
    for k in (1025, 2048):
        assert [group_u8(k, Dp, 16) for Dp in (1920, 1952, 2048)] == [4, 2, 2]
        assert group_u8(k, 1936, 16) == 4 and group_u8(k, 1937, 16) == 2            # the edge itself: Dp <= 1936
    assert group_u8(512, 2048, 16) == 8 and group_u8(100, 2048, 16) == 16 and group_u8(100, 160, 8) == 8
    assert all(D % 32 == 0 for D in (160, 1920, 1952, 2048)) and 160 % 64 == 32 and 160 // 64 == 2 and 1952 % 64 == 32
    assert sorted({cap_of(k) for k in KS}) == [512, 1024, 2048, 4096] and LONG > 4096 - 256 and EQUAL > 1024 - 256
    assert slices_of(2049, 1, 10)[0] == 2048 and slices_of(33, 1024, 2048) == (16, 8) and 33 - 2 * 16 == 1
    assert (2048 * 160) % 16 == 0 and (16 * 32) % 16 == 0                           # a slice's queries stay 16-byte aligned


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_sink_case_is_what_it_is_built_to_be(kind):
    c = sink_case(kind)
    long_rows, equal_rows = c["rows"][:LONG], c["rows"][LONG:LONG + EQUAL]
    by_run = np.concatenate([long_rows[r:r + 18] for r in range(LONG - 18, -1, -18)])   # the last run first, ids ascending in it
    for k in KS:
        ids, dists = c["alone"][0][k]
        for q in range(8):
            assert np.array_equal(ids[q], by_run[:k]) and np.all(np.diff(dists[q]) >= 0)
        for q in range(8, 16):
            assert np.array_equal(ids[q], long_rows[:k]) and np.all(np.diff(dists[q]) >= 0)
        assert len(np.unique(dists[0])) >= k // 18 and not np.array_equal(dists[0], dists[1])
        assert np.array_equal(c["alone"][1][k][0][3, :min(k, EQUAL)], equal_rows[:k])   # the k lowest ids
        far = c["alone"][2][k]
        assert far[1][0][0] > dists[0][k - 1] and (far[0][0] >= 0).sum() == 50      # above list 0's last threshold; alone: all there
    for l, (k, (length, run)) in enumerate(LATE.items(), 5):
        late = c["rows"][c["offsets"][l]:c["offsets"][l + 1]]
        ids = c["alone"][l][k][0][8]
        assert length > cap_of(k) and ids[k - 1] == late[-1] and np.array_equal(ids[:k - 1], late[:k - 1])  # the k-th comes last


# ---- 10. width -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("G", [None, 16], ids=["shipped", "G16"])
@pytest.mark.parametrize("D", [160, 2048])
def test_wide_rows_in_full_blocks_and_tiles(gpu, monkeypatch, D, G, kind):
    """D = 160: two K steps and a half one behind them.  D = 2048: 32 steps of prefetch with all four blocks of a wavefront
    live, all-0 and all-255 rows and queries inside a full tile."""
    import torch
    if G is not None:
        with_group(monkeypatch, G)
    c = wide_case(kind, D)
    assert c["want"][1][48, 65] == F32(D * 255 ** 2) and c["want"][0][48, 66] == -1  # lists 7 and 1: 66 rows, the farthest last
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        assert FR.same(ivf.search_probes(c["qs"], c["probes"], 100), c["want"]), (kind, D, G)
        assert FR.same(host(ivf.search_probes_torch(*device(torch, c["qs"], c["probes"]), 100)), c["want"]), (kind, D, G, "device")


# ---- 11. groups the LDS leaves -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("top_k", [1025, 2048])
@pytest.mark.parametrize("D", [1920, 1952, 2048])
def test_wide_rows_beside_a_large_top_k(gpu, monkeypatch, D, top_k, kind):
    """Asked for G = 16 at cap 4096: G = 4 up to Dp = 1936, G = 2 beyond."""
    with_group(monkeypatch, 16)
    c = lds_case(kind, D)
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        assert FR.same(ivf.search_probes(c["qs"], c["probes"], top_k), c["want"][top_k]), (kind, D, top_k)


# ---- 12. the sink and slices -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("G", [16, 4, None], ids=["G16", "G4", "shipped"])
def test_the_sink_is_cut_at_every_buffer_size(gpu, monkeypatch, G, kind):
    if G is not None:
        with_group(monkeypatch, G)
    c = sink_case(kind)
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        for k in KS:
            assert FR.same(ivf.search_probes(c["qs"], c["probes"], k), c["want"][k]), (kind, G, k)
        for l in ALONE:
            for k in KS:
                assert FR.same(ivf.search_probes(c["qs"], np.full((16, 1), l, dtype=np.int32), k), c["alone"][l][k]), (kind, G, l, k)


def three_lists(kind, D=4):
    rng = np.random.default_rng(4)
    c = dict(kind=kind, base=as_kind(kind, rng.integers(0, 256, (300, D))), labels=(np.arange(300) % 4 - 1).astype(np.int32), nlist=3,
             qs=as_kind(kind, rng.integers(0, 256, (2049, D))))
    c["offsets"], c["rows"] = FR.lists_from_labels(c["labels"], 3)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_two_slices_of_queries(gpu, kind):
    """nq = 2049 at nprobe 1, top_k 10: the second slice's queries and norms start at q0 = 2048.  The norms of the queries
    differ, so a norm read from another query shows."""
    c = three_lists(kind)
    probes = (np.arange(2049) % 3).astype(np.int32)[:, None]
    want = FR.search(c, c["qs"], probes, 10)
    assert not FR.same((want[0][-1:], want[1][-1:]), FR.search(c, c["qs"][:1], probes[-1:], 10))
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        got = ivf.search_probes(c["qs"], probes, 10)
        assert FR.same((got[0][-1:], got[1][-1:]), FR.search(c, c["qs"][-1:], probes[-1:], 10)), "the last query, alone in its slice"
        assert FR.same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_whole_search_across_a_slice_boundary(gpu, kind):
    """search at nq = 2049 is probe followed by search_probes, host and device forms."""
    import torch
    c = three_lists(kind)
    cents = np.random.default_rng(5).integers(0, 256, (3, 4)).astype(F32) - KINDS[kind][1]
    flat, ivf = open_bytes(gpu, c, centroids=cents)
    with flat, ivf:
        lists, _ = ivf.probe(c["qs"], 2)
        assert len({tuple(row) for row in lists}) > 1
        want = FR.search(c, c["qs"], lists, 10)
        assert FR.same(ivf.search_probes(c["qs"], lists, 10), want) and FR.same(ivf.search(c["qs"], 2, 10), want)
        assert FR.same(host(ivf.search_torch(device(torch, c["qs"])[0], 2, 10)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_slices_of_sixteen_queries(gpu, kind):
    """nq = 33 at nlist = nprobe = 1024, top_k 2048: slices of 16, 16 and 1 query; every row is labelled and every list
    probed, so the answer is the exact search's."""
    n, nlist = 6000, 1024
    rng = np.random.default_rng(91)
    c = dict(kind=kind, base=as_kind(kind, rng.integers(0, 256, (n, 5))), labels=rng.integers(0, nlist, size=n).astype(np.int32),
             nlist=nlist, qs=as_kind(kind, rng.integers(0, 256, (33, 5))))
    c["offsets"], c["rows"] = FR.lists_from_labels(c["labels"], nlist)
    probes = np.stack([rng.permutation(nlist) for _ in range(33)]).astype(np.int32)
    want = FR.search(c, c["qs"], probes, 2048)
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        got = ivf.search_probes(c["qs"], probes, 2048)
        assert FR.same(got, want) and FR.same(got, flat.search(c["qs"], 2048))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_device_queries_off_their_alignment(gpu, kind):
    """Device queries one byte off any alignment equal the aligned call."""
    import torch
    c = wide_case(kind, 160)
    t_q, t_p = device(torch, c["qs"], c["probes"])
    buf = torch.zeros(T.NQ * 160 + 16, dtype=t_q.dtype).cuda()
    buf[1:1 + T.NQ * 160] = t_q.ravel()
    moved = buf[1:1 + T.NQ * 160].view(T.NQ, 160)
    assert moved.data_ptr() % 16 == 1 and t_q.data_ptr() % 16 == 0 and moved.is_contiguous()
    flat, ivf = open_bytes(gpu, c)
    with flat, ivf:
        assert FR.same(host(ivf.search_probes_torch(t_q, t_p, 100)), c["want"])
        assert FR.same(host(ivf.search_probes_torch(moved, t_p, 100)), c["want"])
