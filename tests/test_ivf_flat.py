"""IVF search over raw vectors (include/deltapq_amd.h "IVF search over raw vectors").  The reference is the numpy
restatement of tests/_flat_ivf_restatement.py -- fp32 subtract and square, a float64 sum in dimension order, one cast --
restricted to the union of the probed lists.  The GPU meets it bit for bit, for every group size G of the scan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from _flat_ivf_restatement import distances, lists_from_labels, same, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_flat_ivf_create", "dpq_flat_ivf_create_device", "dpq_flat_ivf_build", "dpq_flat_ivf_set_centroids",
           "dpq_flat_ivf_get_info", "dpq_flat_ivf_get", "dpq_flat_ivf_probe", "dpq_flat_ivf_search_probes",
           "dpq_flat_ivf_search_probes_device", "dpq_flat_ivf_search", "dpq_flat_ivf_search_device")
F32, F64 = np.float32, np.float64
# lists 0 .. 11: the row-tile edge; 5 is long with its nearest rows last; 6 .. 8 are short and far; row 0 is in no list
LENGTHS = (0, 1, 255, 256, 257, 1500, 40, 30, 20, 300, 300, 300)
NLIST, NQ = len(LENGTHS), 50


_cases = {}


def make_case(D):
    """One base with its lists, built once per D and left unchanged."""
    if D in _cases:
        return _cases[D]
    rng = np.random.default_rng(D)
    n = sum(LENGTHS) + 37
    labels = np.full(n, -1, dtype=np.int32)
    labels[1 + rng.permutation(n - 1)[:sum(LENGTHS)]] = np.repeat(np.arange(NLIST), LENGTHS)
    offsets, rows = lists_from_labels(labels, NLIST)
    base = rng.standard_normal((n, D)).astype(F32)
    of = lambda l: rows[offsets[l]:offsets[l + 1]]
    far = (3.0 + 0.01 * (LENGTHS[5] - np.arange(LENGTHS[5]))).astype(F32)          # list 5: every tile beats the one before
    base[of(5)] = far[:, None] * np.ones(D, dtype=F32) + F32(1e-4) * base[of(5)]
    for l in (6, 7, 8):
        base[of(l)] += F32(50)
    base[of(4)[1::2]] = base[of(4)[0:-1:2]]                                        # equal distances: the id decides
    cents = rng.standard_normal((NLIST, D)).astype(F32)
    cents[1] = cents[0]                                                            # a tie: the lower list number first
    q = np.arange(NQ)
    col0 = np.select([q < 17, q < 33, q < 48, q < 49], [5, 4, 3, 2], 1)            # 17, 16, 15, 1 and 1 queries per list
    probes = np.stack([col0, 6 + q % 3, np.where(q % 2 == 0, -1, 9 + q % 3), np.where(q % 5 == 0, col0, q % 2 * 10)], 1)
    c = dict(D=D, base=base, labels=labels, offsets=offsets, rows=rows, cents=cents, probes=probes.astype(np.int32),
             qs=(F32(0.1) * rng.standard_normal((NQ, D))).astype(F32))
    _cases[D] = c
    return c


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def open_case(api, c, id_offset=0, centroids=True):
    flat = api.FlatIndex(c["base"], id_offset=id_offset)
    return flat, api.FlatIVF.from_labels(flat, c["labels"], NLIST, centroids=c["cents"] if centroids else None)


def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS + ("dpq_flat_ivf_free",):
        assert re.search(r"\b(int|void) %s\(" % name, header), name + " is not declared"
        assert name in exported and name in bound and hasattr(lib, name), name


def test_argument_errors_come_before_any_device_call(lib):
    fake = ctypes.c_void_p(0x1000)                                                 # never dereferenced: the checks come first
    q, p = np.zeros((2, 4), dtype=F32), np.zeros((2, 1), dtype=np.int32)
    ids, dists = np.zeros((2, 2048), dtype=np.int32), np.zeros((2, 2048), dtype=F32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p()
    assert lib.dpq_flat_ivf_create(None, ptr(p), 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create(fake, None, 2, 1, out) == ERR_ARG
    assert lib.dpq_flat_ivf_create(fake, ptr(p), 2, 0, out) == ERR_ARG and lib.dpq_flat_ivf_build(fake, ptr(q), 65537, out) == ERR_ARG
    assert lib.dpq_flat_ivf_search(None, ptr(q), 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search(fake, None, 2, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_search_probes(fake, ptr(q), 2, None, 1, 1, ptr(ids), ptr(dists)) == ERR_ARG
    for nq, nprobe, top_k in ((-1, 1, 1), (2, 0, 1), (2, 1025, 1), (2, 1, 0), (2, 1, 2049)):
        assert lib.dpq_flat_ivf_search(fake, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
        assert lib.dpq_flat_ivf_search_probes(fake, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists)) == ERR_ARG
    assert lib.dpq_flat_ivf_probe(fake, ptr(q), 2, 0, ptr(ids), None) == ERR_ARG
    assert lib.dpq_flat_ivf_get_info(None, None) == ERR_ARG and lib.dpq_flat_ivf_free(None) is None


@pytest.mark.parametrize("D", [3, 128])
def test_the_restatement_is_within_its_bound_of_float64(D):
    """A term carries three fp32 roundings -- the difference (twice: it is squared) and the square -- and the sum one more:
    a relative error of at most 4 u plus second-order terms, below 5 u, u = 2^-24.  Every term is non-negative, so the
    bound on the terms is a bound on the sum; the float64 sum's own error, D * 2^-53, is far below u at these D."""
    rng = np.random.default_rng(D)
    rows, q = rng.standard_normal((500, D)).astype(F32), rng.standard_normal(D).astype(F32)
    exact = ((rows.astype(F64) - q.astype(F64)) ** 2).sum(axis=1)
    assert np.all(np.abs(distances(rows, q).astype(F64) - exact) <= 5 * 2.0 ** -24 * exact)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 32, 33, 128])
def test_probed_lists_give_the_restated_answer(gpu, D):
    """Every list length of the tile edge, the long list whose buffer is cut again and again, 0 to G + 1 queries per list,
    runs that span many lists and end in padding, -1 and repeated probes, duplicated rows, a non-zero id_offset; host
    and device forms."""
    import torch
    c = make_case(D)
    off = 1000 if D == 33 else 0
    flat, ivf = open_case(gpu, c, id_offset=off)
    with flat, ivf:
        want = search(c, c["qs"], c["probes"], 100, id_offset=off)
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), want)
        got = ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(c["probes"]).cuda(), 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.gpu
@pytest.mark.parametrize("top_k,nprobe", [(1, 4), (257, 4), (2048, 9), (700, 2)])
def test_top_k_from_one_to_the_limit(gpu, monkeypatch, top_k, nprobe):
    """Asked for G = 16.  257: P2 doubles and G shrinks to 8.  2048 with nprobe 9: G = 2 and two merge rounds.  700 over
    lists 0 .. 2: more than the union holds, so padding."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", "16")
    c = make_case(32)
    q = np.arange(NQ)
    probes = (np.stack([(3 + q + j) % NLIST for j in range(nprobe)], 1) if nprobe > 2 else np.stack([q % 3, (q + 1) % 3], 1))
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], probes, top_k), search(c, c["qs"], probes, top_k))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 4, 16])
def test_the_answer_does_not_depend_on_the_group(gpu, monkeypatch, G):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    c = make_case(32)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), search(c, c["qs"], c["probes"], 100))


@pytest.mark.gpu
def test_two_slices_of_queries(gpu):
    rng = np.random.default_rng(4)
    c = dict(base=rng.standard_normal((300, 4)).astype(F32), labels=(np.arange(300) % 4 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 3)
    qs, probes = rng.standard_normal((2049, 4)).astype(F32), (np.arange(2049) % 3).astype(np.int32)[:, None]
    with gpu.FlatIndex(c["base"]) as flat, gpu.FlatIVF.from_labels(flat, c["labels"], 3) as ivf:
        assert same(ivf.search_probes(qs, probes, 10), search(c, qs, probes, 10))


@pytest.mark.gpu
def test_the_coarse_step_and_the_whole_search(gpu):
    import torch
    c = make_case(33)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        lists, dists = ivf.probe(c["qs"], 5)
        d = np.stack([distances(c["cents"], q) for q in c["qs"]])
        order = np.stack([np.lexsort((np.arange(NLIST), row))[:5] for row in d])   # by (distance, list number)
        assert np.array_equal(lists, order) and np.array_equal(dists.view(np.uint32), np.take_along_axis(d, order, 1).view(np.uint32))
        assert all(list(row).index(0) + 1 == list(row).index(1) for row in lists if 0 in row[:-1])  # the tie
        want = search(c, c["qs"], lists, 100)
        assert same(ivf.search(c["qs"], 5, 100), want)
        got = ivf.search_torch(torch.from_numpy(c["qs"]).cuda(), 5, 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.gpu
def test_it_agrees_with_the_filtered_exact_search_and_with_ivf_assign(gpu):
    c = make_case(32)
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf:
        offsets, ids = ivf.lists()
        assert np.array_equal(offsets, c["offsets"]) and np.array_equal(ids, c["rows"] + 7)
        inf = ivf.info()
        assert (inf["n_assigned"], inf["n_unassigned"], inf["max_list_len"], inf["has_centroids"]) == (sum(LENGTHS), 37, 1500, 1)
        probes = np.array([[5, 2, 7]], dtype=np.int32)
        union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
        with gpu.FlatIdFilter.from_ids(flat, union + 7) as filt:
            assert same(ivf.search_probes(c["qs"][:1], probes, 100), flat.search_filtered(c["qs"][:1], 100, filt))
        with gpu.FlatIVF.build(flat, c["cents"]) as built:
            labels, _ = gpu.ivf_assign(c["cents"], c["base"])
            want = lists_from_labels(labels, NLIST)
            got = built.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1] + 7)


@pytest.mark.gpu
def test_what_is_refused(gpu):
    c = make_case(32)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    with gpu.FlatIndexU8(np.zeros((8, 4), dtype=np.uint8)) as bytes_index:
        assert status(lambda: gpu.FlatIVF.from_labels(bytes_index, np.zeros(8, dtype=np.int32), 2)) == ERR_ARG
    flat, ivf = open_case(gpu, c, centroids=False)
    with flat, ivf:
        assert status(lambda: gpu.FlatIVF.from_labels(flat, np.where(c["labels"] == 3, NLIST, c["labels"]), NLIST)) == ERR_ARG
        assert status(lambda: gpu.FlatIVF.from_labels(flat, c["labels"][:-1], NLIST)) == ERR_ARG
        assert status(lambda: ivf.search_probes(c["qs"], np.full((NQ, 1), NLIST), 10)) == ERR_ARG
        assert status(lambda: ivf.search(c["qs"], 2, 10)) == ERR_STATE and status(lambda: ivf.probe(c["qs"], 2)) == ERR_STATE
        import torch
        bad = torch.full((NQ, 1), NLIST, dtype=torch.int32).cuda()                 # the device form: the flag word
        assert status(lambda: ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), bad, 10)) == ERR_ARG
        assert same(ivf.search_probes(c["qs"], c["probes"], 10), search(c, c["qs"], c["probes"], 10))  # the next call works
