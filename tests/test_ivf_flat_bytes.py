"""IVF search over byte vectors (include/deltapq_amd.h "IVF search over byte vectors").  The reference is
the numpy restatement of tests/_flat_ivf_restatement.py -- the int64 sum of (v - q)^2 over the rows of the probed lists,
cast once to float32, the keys sorted.  It is exact, so there is no tolerance: ids and distance bits are equal, for every
group size G."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _flat_ivf_restatement import lists_from_labels, same, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_flat_ivf_create_bytes", "dpq_flat_ivf_create_bytes_device", "dpq_flat_ivf_build_bytes", "dpq_flat_ivf_probe_bytes",
           "dpq_flat_ivf_search_probes_bytes", "dpq_flat_ivf_search_probes_bytes_device", "dpq_flat_ivf_search_bytes",
           "dpq_flat_ivf_search_bytes_device")
F32 = np.float32
# lists 0 .. 14: the MFMA block, wavefront and tile edges; 11 is long with its nearest rows last; 12 .. 14 are short and
# far; row 0 is in no list
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1500, 40, 30, 20)
NLIST, NQ, LONG = len(LENGTHS), 50, 11
KINDS = {"u8": (np.uint8, 0), "i8": (np.int8, 128)}                                # dtype, what the values 0 .. 255 are lowered by


_cases = {}


def make_case(kind, D):
    """One base with its lists, built once per (kind, D) and left unchanged."""
    if (kind, D) in _cases:
        return _cases[kind, D]
    dtype, lower = KINDS[kind]
    rng = np.random.default_rng(D)
    n = sum(LENGTHS) + 37
    labels = np.full(n, -1, dtype=np.int32)
    labels[1 + rng.permutation(n - 1)[:sum(LENGTHS)]] = np.repeat(np.arange(NLIST), LENGTHS)
    offsets, rows = lists_from_labels(labels, NLIST)
    base = rng.integers(0, 256, (n, D))
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    base[of(LONG)] = (130 - np.arange(LENGTHS[LONG]) // 12)[:, None]               # every tile beats the one before
    base[of(LONG), rng.integers(0, D, LENGTHS[LONG])] += rng.integers(0, 3, LENGTHS[LONG])
    for l in (12, 13, 14):
        base[of(l)] = 200 + base[of(l)] % 56
    base[of(10)[1::2]] = base[of(10)[0:-1:2]]                                      # equal distances: the id decides
    cents = rng.integers(0, 256, (NLIST, D)).astype(F32) - lower
    cents[1] = cents[0]                                                            # a tie: the lower list number first
    q = np.arange(NQ)
    col0 = np.select([q < 17, q < 33, q < 48, q < 49], [LONG, 10, 9, 8], 1)        # 17, 16, 15, 1 and 1 queries per list
    probes = np.stack([col0, 1 + q % 8, np.where(q % 2 == 0, -1, 12 + q % 3), np.where(q % 5 == 0, col0, q % 2 * 7)], 1)
    as_kind = lambda a: (a - lower).astype(dtype)
    c = dict(kind=kind, D=D, base=as_kind(base), labels=labels, offsets=offsets, rows=rows, cents=cents,
             probes=probes.astype(np.int32), qs=as_kind(rng.integers(0, 40, (NQ, D))))
    _cases[kind, D] = c
    return c


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def open_case(api, c, id_offset=0, centroids=True):
    flat = (api.FlatIndexU8 if c["kind"] == "u8" else api.FlatIndexI8)(c["base"], id_offset=id_offset)
    return flat, api.FlatIVFBytes.from_labels(flat, c["labels"], NLIST, centroids=c["cents"] if centroids else None)


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
    assert lib.dpq_flat_ivf_create_bytes(None, ptr(p), 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bytes(fake, None, 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bytes(fake, ptr(p), 2, 0, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create_bytes_device(fake, ptr(p), -1, 1, None, out) == ERR_ARG
    assert lib.dpq_flat_ivf_build_bytes(fake, ptr(dists), 65537, out) == ERR_ARG
    assert lib.dpq_flat_ivf_search_bytes(None, ptr(q), 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search_bytes(fake, None, 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search_probes_bytes(fake, ptr(q), 2, None, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    for nq, nprobe, top_k in ((-1, 1, 1), (2, 0, 1), (2, 1025, 1), (2, 1, 0), (2, 1, 2049)):
        assert lib.dpq_flat_ivf_search_bytes(fake, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
        assert lib.dpq_flat_ivf_search_bytes_device(fake, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists), None) == ERR_ARG
        assert lib.dpq_flat_ivf_search_probes_bytes(fake, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
        assert lib.dpq_flat_ivf_search_probes_bytes_device(fake, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists),
                                                           None) == ERR_ARG
    assert lib.dpq_flat_ivf_probe_bytes(fake, ptr(q), 2, 0, ptr(ids), None) == ERR_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("D", [3, 32, 33, 96, 128])
def test_probed_lists_give_the_restated_answer(gpu, kind, D):
    """Dp 32 (half a K step alone), 64, 96 (one and a half) and 128; every list length of the block, wavefront and tile
    edges, the long list whose buffer is cut again and again; 0, 1, 15, 16 and 17 queries per list; -1 and repeated
    probes, duplicated rows, a non-zero id_offset; host and device forms."""
    import torch
    c = make_case(kind, D)
    off = 1000 if D == 33 else 0
    flat, ivf = open_case(gpu, c, id_offset=off)
    with flat, ivf:
        want = search(c, c["qs"], c["probes"], 100, id_offset=off)
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), want)
        got = ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(c["probes"]).cuda(), 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_widest_rows_at_the_extreme_values(gpu, kind):
    """D = 2048: 2048 * 255^2 needs the int32 range and rounds above 2^24; the largest Qs."""
    dtype, lower = KINDS[kind]
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (40, 2048))
    base[0:8], base[8:16] = 255, 0
    qs = np.stack([np.zeros(2048, dtype=np.int64), np.full(2048, 255), rng.integers(0, 256, 2048)])
    c = dict(base=(base - lower).astype(dtype), labels=(np.arange(40) % 3 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 2)
    qs, probes = (qs - lower).astype(dtype), np.array([[0, 1], [1, 0], [1, -1]], dtype=np.int32)
    cls = gpu.FlatIndexU8 if kind == "u8" else gpu.FlatIndexI8
    with cls(c["base"]) as flat, gpu.FlatIVFBytes.from_labels(flat, c["labels"], 2) as ivf:
        want = search(c, qs, probes, 30)
        assert want[1][0, 25] == F32(2048 * 255 ** 2) and same(ivf.search_probes(qs, probes, 30), want)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("top_k", [1, 100, 257, 2048])
def test_top_k_from_one_to_the_limit(gpu, monkeypatch, kind, top_k):
    """Asked for G = 16 with nprobe 9.  257: P2 doubles.  2048: the LDS forces G down to 4; nine lists hold fewer rows
    than 2048 for some queries, so padding."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", "16")
    c = make_case(kind, 32)
    probes = np.stack([(3 + np.arange(NQ) + j) % NLIST for j in range(9)], 1)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], probes, top_k), search(c, c["qs"], probes, top_k))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("G", [1, 2, 4, 16])
def test_the_answer_does_not_depend_on_the_group(gpu, monkeypatch, kind, G):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    c = make_case(kind, 96)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), search(c, c["qs"], c["probes"], 100))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_it_agrees_with_what_the_library_already_has(gpu, kind):
    """The byte index's filtered search, the fp32 FlatIVF over the widened rows and queries, its probe, ivf_assign."""
    import torch
    c = make_case(kind, 33)
    wide, wq = c["base"].astype(F32), c["qs"].astype(F32)
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf, gpu.FlatIndex(wide, id_offset=7) as f32:
        probes = np.array([[LONG, 2, 13]], dtype=np.int32)
        union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
        with gpu.FlatIdFilter.from_ids(flat, union + 7) as filt:
            assert same(ivf.search_probes(c["qs"][:1], probes, 100), flat.search_filtered(c["qs"][:1], 100, filt))
        with gpu.FlatIVF.from_labels(f32, c["labels"], NLIST, centroids=c["cents"]) as ivf32:
            assert same(ivf.search_probes(c["qs"], c["probes"], 100), ivf32.search_probes(wq, c["probes"], 100))
            lists = ivf.probe(c["qs"], 5)
            assert same(lists, ivf32.probe(wq, 5))
            assert all(list(row).index(0) + 1 == list(row).index(1) for row in lists[0] if 0 in row[:-1])  # the tie
            want = ivf32.search(wq, 5, 100)
            assert same(ivf.search(c["qs"], 5, 100), want) and same(want, search(c, c["qs"], lists[0], 100, id_offset=7))
            got = ivf.search_torch(torch.from_numpy(c["qs"]).cuda(), 5, 100)
            assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        with gpu.FlatIVFBytes.build(flat, c["cents"]) as built:
            want = lists_from_labels(gpu.ivf_assign(c["cents"], wide)[0], NLIST)
            got = built.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1] + 7)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_what_is_refused(gpu, kind):
    import torch
    c = make_case(kind, 32)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    zeros = np.zeros(8, dtype=np.int32)
    with gpu.FlatIndex(np.zeros((8, 4), dtype=F32)) as f32, gpu.FlatIndexBits(np.zeros((8, 4), dtype=np.uint8), 32) as bits:
        assert status(lambda: gpu.FlatIVFBytes.from_labels(f32, zeros, 2)) == ERR_ARG
        assert status(lambda: gpu.FlatIVFBytes.from_labels(bits, zeros, 2)) == ERR_ARG
        with gpu.FlatIVF.from_labels(f32, zeros, 2) as ivf32:                      # a _bytes search on an fp32 structure
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
            out = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=F32)
            assert ivf32._lib.dpq_flat_ivf_search_probes_bytes(ivf32._h, ptr(np.zeros((1, 4), dtype=np.uint8)), 1, ptr(zeros), 1, 1,
                                                               ptr(out[0]), ptr(out[1])) == ERR_ARG
    flat, ivf = open_case(gpu, c, centroids=False)
    with flat, ivf:
        assert status(lambda: gpu.FlatIVF.search_probes(ivf, c["qs"], c["probes"], 10)) == ERR_ARG  # an fp32 search on a byte one
        assert status(lambda: ivf.search(c["qs"], 2, 10)) == ERR_STATE and status(lambda: ivf.probe(c["qs"], 2)) == ERR_STATE
        assert status(lambda: ivf.search_probes(c["qs"], np.full((NQ, 1), NLIST), 10)) == ERR_ARG
        bad = torch.full((NQ, 1), NLIST, dtype=torch.int32).cuda()                 # the device form: the flag word
        assert status(lambda: ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), bad, 10)) == ERR_ARG
        with pytest.raises(TypeError):
            ivf.search_probes(c["qs"].astype(F32), c["probes"], 10)
        with pytest.raises(TypeError):
            ivf.search_probes_torch(torch.zeros((NQ, 32)).cuda(), bad, 10)
        assert same(ivf.search_probes(c["qs"], c["probes"], 10), search(c, c["qs"], c["probes"], 10))  # the next call works
