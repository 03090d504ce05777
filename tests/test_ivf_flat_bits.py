"""IVF search over binary vectors (include/deltapq_amd.h "IVF search over binary vectors").  The reference is
plain numpy: the bits unpacked, the integer Hamming distance, one cast to float32, the keys (distance bits << 32 | id) of the
probed lists' rows sorted and cut (tests/_flat_ivf_restatement.py for lists, cutting and comparing).  Distances are exact
integers, so there is no tolerance: ids and distance bits are equal, for every group size G.  Ties are dense at small D; at
D = 1 almost every order is decided by the id alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _flat_ivf_restatement import cut, lists_from_labels, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_flat_ivf_create_bits", "dpq_flat_ivf_create_bits_device", "dpq_flat_ivf_build_bits",
           "dpq_flat_ivf_set_centroids_bits", "dpq_flat_ivf_probe_bits", "dpq_flat_ivf_search_bits", "dpq_flat_ivf_search_bits_device",
           "dpq_flat_ivf_search_probes_bits", "dpq_flat_ivf_search_probes_bits_device")
F32 = np.float32
# lists 0 .. 11: the wavefront and tile edges; 8 is long with its nearest rows last; 9 .. 11 are short and far; row 0 is in
# no list
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1500, 40, 30, 20)
NLIST, NQ, LONG = len(LENGTHS), 50, 8

_cases = {}


def pack(b01, dirty=False):
    """[m][D] 0/1 -> uint8 [m][(D + 7) // 8], dimension d in bit d & 7 of byte d >> 3; dirty: the spare bits set."""
    spare = np.full((len(b01), -b01.shape[1] % 8), int(dirty), dtype=np.uint8)
    return np.packbits(np.concatenate([b01, spare], axis=1), axis=1, bitorder="little")


def hamming(rows01, qs01):
    """float32 [nq][n]: the count of differing dimensions, an integer, cast once."""
    return np.stack([(rows01 != q).sum(axis=1) for q in qs01]).astype(F32)


def make_case(D):
    """One base with its lists and every (query, row) distance, built once per D and left unchanged."""
    if D in _cases:
        return _cases[D]
    rng = np.random.default_rng(D)
    n = sum(LENGTHS) + 37
    labels = np.full(n, -1, dtype=np.int32)
    labels[1 + rng.permutation(n - 1)[:sum(LENGTHS)]] = np.repeat(np.arange(NLIST), LENGTHS)
    offsets, rows = lists_from_labels(labels, NLIST)
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    b01 = rng.integers(0, 2, (n, D), dtype=np.uint8)
    ones = D - np.arange(LENGTHS[LONG]) * D // LENGTHS[LONG]                        # the queries are sparse: fewer ones, nearer
    b01[of(LONG)] = np.arange(D)[None, :] < ones[:, None]
    b01[of(LONG), rng.integers(0, D, LENGTHS[LONG])] ^= rng.integers(0, 2, LENGTHS[LONG], dtype=np.uint8)
    for l in (9, 10, 11):
        b01[of(l)] |= rng.integers(0, 8, (LENGTHS[l], D)) > 0
    b01[of(7)[1::2]] = b01[of(7)[0:-1:2]]                                          # equal distances: the id decides
    cents01 = rng.integers(0, 2, (NLIST, D), dtype=np.uint8)
    cents01[:2] = 0                                                                # near the sparse queries, and a tie: the lower list number first
    qs01 = (rng.integers(0, 10, (NQ, D)) == 0).astype(np.uint8)
    q = np.arange(NQ)
    col0 = np.select([q < 17, q < 33, q < 48, q < 49], [LONG, 7, 6, 5], 1)         # 17, 16, 15, 1 and 1 queries per list
    probes = np.stack([col0, 1 + q % 8, np.where(q % 2 == 0, -1, 9 + q % 3), np.where(q % 5 == 0, col0, q % 2 * 4)], 1)
    c = dict(D=D, b01=b01, base=pack(b01, dirty=True), labels=labels, offsets=offsets, rows=rows, cents01=cents01,
             cents=pack(cents01, dirty=True), probes=probes.astype(np.int32), qs01=qs01, qs=pack(qs01),
             qs_dirty=pack(qs01, dirty=True), dist=hamming(b01, qs01))
    _cases[D] = c
    return c


def restated(c, probes, top_k, id_offset=0):
    """(ids int32 [nq][top_k], dists float32 [nq][top_k]): the sorted keys of the union of each query's probed lists, cut."""
    ids, dists = np.empty((len(probes), top_k), dtype=np.int32), np.empty((len(probes), top_k), dtype=F32)
    for i, row in enumerate(probes):
        lists = list(dict.fromkeys(int(p) for p in row if p >= 0))
        r = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in lists] + [np.zeros(0, dtype=np.int64)])
        keys = (c["dist"][i, r].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (r + id_offset).astype(np.uint64)
        ids[i], dists[i] = cut(np.sort(keys), top_k)
    return ids, dists


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def open_case(api, c, id_offset=0, centroids=True):
    flat = api.FlatIndexBits(c["base"], c["D"], id_offset=id_offset)
    return flat, api.FlatIVFBits.from_labels(flat, c["labels"], NLIST, centroids=c["cents"] if centroids else None)


def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared"
        assert name in exported and name in bound and hasattr(lib, name), name


def test_argument_errors_come_before_any_device_call(lib):
    fake = ctypes.c_void_p(0x1000)                                                 # never dereferenced: the checks come first
    q, p = np.zeros((2, 4), dtype=np.uint8), np.zeros((2, 1), dtype=np.int32)
    ids, dists = np.zeros((2, 2048), dtype=np.int32), np.zeros((2, 2048), dtype=F32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p()
    assert lib.dpq_flat_ivf_create_bits(None, ptr(p), 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bits(fake, None, 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bits(fake, ptr(p), 2, 0, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bits_device(fake, ptr(p), -1, 1, None, out) == ERR_ARG
    assert lib.dpq_flat_ivf_build_bits(fake, ptr(q), 65537, out) == ERR_ARG
    assert lib.dpq_flat_ivf_build_bits(fake, None, 2, out) == ERR_ARG
    assert lib.dpq_flat_ivf_set_centroids_bits(fake, None, 2) == ERR_ARG
    assert lib.dpq_flat_ivf_search_bits(None, ptr(q), 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search_bits(fake, None, 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search_probes_bits(fake, ptr(q), 2, None, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    for nq, nprobe, top_k in ((-1, 1, 1), (2, 0, 1), (2, 1025, 1), (2, 1, 0), (2, 1, 2049)):
        assert lib.dpq_flat_ivf_search_bits(fake, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
        assert lib.dpq_flat_ivf_search_bits_device(fake, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists), None) == ERR_ARG
        assert lib.dpq_flat_ivf_search_probes_bits(fake, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
        assert lib.dpq_flat_ivf_search_probes_bits_device(fake, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists),
                                                          None) == ERR_ARG
    assert lib.dpq_flat_ivf_probe_bits(fake, ptr(q), 2, 0, ptr(ids), None) == ERR_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 13, 128, 129, 1024, 4096])
def test_probed_lists_give_the_restated_answer(gpu, D):
    """A lone byte with spare bits, a partial last byte, one 16-byte row, a row one bit over, the 32-word chunks, the limit.
    Every list length of the wavefront and tile edges, the long list whose buffer is cut again and again; 0, 1, 15, 16 and 17
    queries per list; -1 and repeated probes, duplicated rows, a non-zero id_offset; host and device forms.  The rows and
    the centroids are given with their spare bits SET, the queries with them clear and set: they are no dimensions."""
    import torch
    c = make_case(D)
    off = 1000 if D == 129 else 0
    flat, ivf = open_case(gpu, c, id_offset=off)
    with flat, ivf:
        want = restated(c, c["probes"], 100, id_offset=off)
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), want)
        assert same(ivf.search_probes(c["qs_dirty"], c["probes"], 100), want)
        got = ivf.search_probes_torch(torch.from_numpy(c["qs_dirty"]).cuda(), torch.from_numpy(c["probes"]).cuda(), 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        for i in (0, 20, 49):                                                      # the library's own filtered search
            union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in set(c["probes"][i]) - {-1}])
            with gpu.FlatIdFilter.from_ids(flat, union + off) as filt:
                assert same(flat.search_filtered(c["qs"][i:i + 1], 100, filt), (want[0][i:i + 1], want[1][i:i + 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [129, 1024])
@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_the_answer_does_not_depend_on_the_group(gpu, monkeypatch, D, G):
    """Both chunk widths; G also bounds a stretch, so 16 is what reaches the 16-query form of the inner loop."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    c = make_case(D)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), restated(c, c["probes"], 100))


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [1, 100, 256, 257, 2048])
def test_top_k_from_one_to_the_limit(gpu, monkeypatch, top_k):
    """Asked for G = 16 with nprobe 9, the long list among them.  257: P2 doubles.  2048: the LDS forces G down to 4; nine
    lists hold fewer rows than 2048 for some queries, so padding."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", "16")
    c = make_case(128)
    probes = np.stack([(3 + np.arange(NQ) + j) % NLIST for j in range(9)], 1)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        got, want = ivf.search_probes(c["qs"], probes, top_k), restated(c, probes, top_k)
        assert same(got, want) and (top_k < 2048 or (want[0][:, -1] == -1).any())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [13, 1024])
def test_the_coarse_step_ranks_binary_centroids_by_hamming_distance(gpu, D):
    """probe: (distance, list number), lists 0 and 1 being equal; build: the nearest centroid, the lower number at a tie;
    search = probe, then search_probes; no centroids, no coarse step."""
    import torch
    c = make_case(D)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        cd = hamming(c["cents01"], c["qs01"])
        order = np.argsort(cd, axis=1, kind="stable")[:, :5]
        lists, dists = ivf.probe(c["qs_dirty"], 5)
        assert np.array_equal(lists, order) and np.array_equal(dists, np.take_along_axis(cd, order, 1))
        assert all(list(row).index(0) + 1 == list(row).index(1) for row in lists if 0 in row[:-1])
        want = ivf.search_probes(c["qs"], lists, 100)
        assert same(want, restated(c, lists, 100)) and same(ivf.search(c["qs"], 5, 100), want)
        got = ivf.search_torch(torch.from_numpy(c["qs"]).cuda(), 5, 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        with gpu.FlatIVFBits.build(flat, c["cents"]) as built:
            nearest = np.argmin(hamming(c["cents01"], c["b01"]), axis=1).astype(np.int32)  # the first minimum: the lower list
            assert (nearest != 1).all() and built.info()["has_centroids"] == 1
            want = lists_from_labels(nearest, NLIST)
            got = built.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    flat, ivf = open_case(gpu, c, centroids=False)
    with flat, ivf:
        assert status(lambda: ivf.search(c["qs"], 2, 10)) == ERR_STATE and status(lambda: ivf.probe(c["qs"], 2)) == ERR_STATE


@pytest.mark.gpu
def test_every_kind_of_structure_has_its_own_calls(gpu):
    c = make_case(128)                                                             # 16 bytes: also a legal row of 16 bytes or 4 floats
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    zeros = np.zeros(8, dtype=np.int32)
    flat, ivf = open_case(gpu, c, centroids=False)
    with flat, ivf, gpu.FlatIndex(np.zeros((8, 4), dtype=F32)) as f32, gpu.FlatIndexU8(np.zeros((8, 16), dtype=np.uint8)) as u8:
        assert status(lambda: gpu.FlatIVF.from_labels(flat, c["labels"], NLIST)) == ERR_ARG
        assert status(lambda: gpu.FlatIVFBytes.from_labels(flat, c["labels"], NLIST)) == ERR_ARG
        assert status(lambda: gpu.FlatIVF.build(flat, np.zeros((2, 128), dtype=F32))) == ERR_ARG
        assert status(lambda: gpu.FlatIVFBits.from_labels(f32, zeros, 2)) == ERR_ARG
        assert status(lambda: gpu.FlatIVFBits.from_labels(u8, zeros, 2)) == ERR_ARG
        assert status(lambda: gpu.FlatIVF.set_centroids(ivf, np.zeros((NLIST, 128), dtype=F32))) == ERR_ARG
        assert status(lambda: gpu.FlatIVFBytes.search_probes(ivf, c["qs"], c["probes"], 10)) == ERR_ARG
        with gpu.FlatIVFBytes.from_labels(u8, zeros, 2) as ivf8, gpu.FlatIVF.from_labels(f32, zeros, 2) as ivf32:
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            q, out = np.zeros((1, 16), dtype=np.uint8), (np.zeros(1, dtype=np.int32), np.zeros(1, dtype=F32))
            for other in (ivf8, ivf32):                                            # a _bits call on a byte and an fp32 structure
                assert other._lib.dpq_flat_ivf_search_probes_bits(other._h, ptr(q), 1, ptr(zeros), 1, 1, ptr(out[0]),
                                                                  ptr(out[1])) == ERR_ARG
                assert other._lib.dpq_flat_ivf_set_centroids_bits(other._h, ptr(q), 2) == ERR_ARG
        with pytest.raises(TypeError):
            ivf.search_probes(c["qs"].astype(F32), c["probes"], 10)
        assert same(ivf.search_probes(c["qs"], c["probes"], 10), restated(c, c["probes"], 10))  # the next call works
