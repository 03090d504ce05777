"""IVF search (dpq_ivf_*): inverted lists over a handle's nodes, built on the device from labels or from centroids, and
the search over the lists each query probes.

GPU: strictly (ids and distance bits, every query) against the exact-rational reference of tests/_numeric_edges.py, through
the restatement of tests/_ivf_restatement.py, and against query_batch on the same handle; list lengths around the stride
of 256, the threshold refresh of the scan's buffer, the merge rounds, padding, the flag words, ids on shards, parts, even-N
and prefix handles, the build from centroids, the state a call leaves behind, the CLI.  CPU: the symbols, the hand case,
the probe rule, the argument checks.  Nothing is skipped and no case is exempt.
Every open option: tests/test_matrix_ivf.py; slices, merge rounds, long probe rows, the sort width: tests/test_ivf_edges.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _candidates_restatement as C
import _ivf_restatement as R
import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_ivf_create", "dpq_ivf_create_device", "dpq_ivf_build", "dpq_ivf_set_centroids", "dpq_ivf_free",
           "dpq_ivf_get_info", "dpq_ivf_get", "dpq_ivf_search_probes", "dpq_ivf_search_probes_device", "dpq_ivf_probe",
           "dpq_ivf_search", "dpq_ivf_search_device")
_cache = {}


def built_class(name, M=8, n=ne.N_SCAN):
    """One build per (class, M, n) and module; nobody writes to it."""
    key = (name, M, n)
    if key not in _cache:
        _cache[key] = ne.build_class(name, M, 256, n, plain_rule=True)
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


def queries_of(c, nq):
    use = np.arange(nq) % len(c["queries"])
    return use, np.ascontiguousarray(c["queries"][use])


def rows(lists, width=None, fill=-1):
    width = max(1, max(len(l) for l in lists)) if width is None else width
    out = np.full((len(lists), width), fill, dtype=np.int32)
    for q, l in enumerate(lists):
        out[q, :len(l)] = l
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in bound and hasattr(lib, name), name + " is not bound"
    assert ctypes.sizeof(_lib.IvfStats) == 4 * 8 + 2 * 4


def test_the_hand_case():
    """N = 6 (even, DTC), labels [0, 1, 0, -1, 1, 0]: node 5 is reported as 6, node 3 is in no list.  Distances by
    position [5, 4, 3, 0, 1, 2]: node 3 would win every search and is in none."""
    offsets, ids = R.lists_from_labels([0, 1, 0, -1, 1, 0], 2, even_rule=True)
    assert offsets.tolist() == [0, 3, 5]
    assert ids[0:3].tolist() == [0, 2, 6] and ids[3:5].tolist() == [1, 4]
    d = np.array([5, 4, 3, 0, 1, 2], dtype=np.float32)
    rules = dict(id_base=0, n_local=6, n_total=6, even_rule=True)
    i, dd = R.search_row(d, offsets, ids, [1, -1], 2, **rules)
    assert i.tolist() == [4, 1] and dd.tolist() == [1.0, 4.0]
    i, dd = R.search_row(d, offsets, ids, [0, 1], 2, **rules)
    assert i.tolist() == [4, 6] and dd.tolist() == [1.0, 2.0]
    i, dd = R.search_row(d, offsets, ids, [0, 0], 2, **rules)                  # the duplicate counts once
    assert i.tolist() == [6, 2] and dd.tolist() == [2.0, 3.0]
    i, dd = R.search_row(d, offsets, ids, [0, 0], 4, **rules)
    assert i.tolist() == [6, 2, 0, -1] and dd[:3].tolist() == [2.0, 3.0, 5.0] and np.isposinf(dd[3])
    i, dd = R.search_row(d, offsets, ids, [-1, -1], 2, **rules)
    assert i.tolist() == [-1, -1] and np.all(np.isposinf(dd))
    with pytest.raises(ValueError):
        R.search_row(d, offsets, ids, [2, 0], 2, **rules)
    with pytest.raises(ValueError):
        R.lists_from_labels([0, 2], 2)
    # a plain handle of the same six nodes: no renaming
    _, ids = R.lists_from_labels([0, 1, 0, -1, 1, 0], 2, even_rule=False)
    assert ids.tolist() == [0, 2, 5, 1, 4]
    # the shard [3, 6) of the same index
    offsets, ids = R.lists_from_labels([-1, 1, 0], 2, node_lo=3, n_total=6, even_rule=True)
    assert offsets.tolist() == [0, 1, 2] and ids.tolist() == [6, 4]


def test_the_probe_rule_breaks_ties_by_the_lowest_list():
    cents = np.array([[4, 0], [0, 3], [0, -3], [1, 0], [0, 3]], dtype=np.float32)
    lists, dists = R.probe(cents, np.zeros((1, 2), dtype=np.float32), 5)
    assert lists[0].tolist() == [3, 1, 2, 4, 0] and dists[0].tolist() == [1.0, 9.0, 9.0, 9.0, 16.0]
    assert R.probe(cents, [[0.0, 0.0]], 2)[0][0].tolist() == [3, 1]
    assert R.assign(np.array([[0, 3], [0, 0], [0, -2]], dtype=np.float32), cents).tolist() == [1, 3, 2]


def test_argument_errors_need_no_device(lib):
    """NULL pointers and the bounds of top_k, nprobe and nq are refused before the handle is looked at (the handle below
    is never dereferenced) and before a device is asked for."""
    buf = np.zeros(64, dtype=np.float32)
    ib = np.zeros(64, dtype=np.int32)
    p, ip, h = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ib.ctypes.data), ctypes.c_void_p(0x1000)
    for fn, tail in ((lib.dpq_ivf_search_probes, ()), (lib.dpq_ivf_search_probes_device, (None,))):
        assert fn(None, p, 1, ip, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, None, 1, ip, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, None, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, ip, 2, 2, None, p, *tail) == ERR_ARG
        assert fn(h, p, 1, ip, 2, 2, ip, None, *tail) == ERR_ARG
        assert fn(h, p, -1, ip, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, ip, 2, 0, ip, p, *tail) == ERR_ARG                 # top_k
        assert fn(h, p, 1, ip, 2, 2049, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, ip, 0, 2, ip, p, *tail) == ERR_ARG                 # nprobe
        assert fn(h, p, 1, ip, 1025, 2, ip, p, *tail) == ERR_ARG
    for fn, tail in ((lib.dpq_ivf_search, ()), (lib.dpq_ivf_search_device, (None,))):
        assert fn(None, p, 1, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, None, 1, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 2, 2, None, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 2, 2, ip, None, *tail) == ERR_ARG
        assert fn(h, p, -1, 2, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 2, 0, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 2, 2049, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 0, 2, ip, p, *tail) == ERR_ARG
        assert fn(h, p, 1, 1025, 2, ip, p, *tail) == ERR_ARG
    assert lib.dpq_ivf_probe(None, p, 1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe(h, None, 1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe(h, p, 1, 2, None, p) == ERR_ARG
    assert lib.dpq_ivf_probe(h, p, -1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe(h, p, 1, 0, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe(h, p, 1, 1025, ip, p) == ERR_ARG
    assert b"dpq_ivf_probe" in lib.dpq_last_error()
    out = ctypes.c_void_p(0x2000)
    assert lib.dpq_ivf_create(None, ip, 4, 2, out) == ERR_ARG and out.value is None   # *out is cleared
    assert lib.dpq_ivf_create(h, None, 4, 2, out) == ERR_ARG
    assert lib.dpq_ivf_create(h, ip, 4, 2, None) == ERR_ARG
    assert lib.dpq_ivf_create(h, ip, -1, 2, out) == ERR_ARG
    assert lib.dpq_ivf_create(h, ip, 4, 0, out) == ERR_ARG
    assert lib.dpq_ivf_create(h, ip, 4, 65537, out) == ERR_ARG
    ib[2] = 2
    assert lib.dpq_ivf_create(h, ip, 4, 2, out) == ERR_ARG                      # a label >= nlist, on the host
    ib[2] = 0
    assert lib.dpq_ivf_create_device(h, None, 4, 2, None, out) == ERR_ARG
    assert lib.dpq_ivf_create_device(h, ip, 4, 65537, None, out) == ERR_ARG
    assert lib.dpq_ivf_build(h, None, 2, out) == ERR_ARG
    assert lib.dpq_ivf_build(h, p, 0, out) == ERR_ARG
    assert lib.dpq_ivf_set_centroids(None, p, 2) == ERR_ARG
    assert lib.dpq_ivf_get_info(None, None) == ERR_ARG
    assert lib.dpq_ivf_get(None, None, None) == ERR_ARG
    lib.dpq_ivf_free(None)                                                      # nothing happens


# ---- 1. equivalence with the exhaustive search ------------------------------------------------------------------------------

HANDLES = {"dtc_m8": (8, False), "dtc_m16": (16, False), "plain_m8": (8, True), "plain_m16": (16, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [ne.SMALL_N, ne.N_SCAN])
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", ["fp32_ties", "ulp_crowd", "constant", "overflow"])
def test_every_list_probed_is_the_exhaustive_search(gpu, name, handle, n):
    """nprobe = nlist and every node labelled: the answer is query_batch's on the same handle, bit for bit, and the
    exact-rational reference's -- tie groups across the k-th boundary, real ids at +inf, and at top_k > n the real ids at
    +inf in front of the padding."""
    M, plain = HANDLES[handle]
    c = built_class(name, M, n)
    alld = c["d32"] if plain else c["d64"]
    nq, nlist = 5, 7
    use, qs = queries_of(c, nq)
    rng = np.random.default_rng(n + M)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    probes = np.stack([rng.permutation(nlist) for _ in range(nq)]).astype(np.int32)
    with open_class(gpu, c, plain) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        inf = ivf.info()
        assert (inf["nlist"], inf["n_assigned"], inf["n_unassigned"], inf["has_centroids"]) == (nlist, n, 0, 0)
        assert inf["max_list_len"] == np.bincount(labels, minlength=nlist).max()
        assert inf["device_bytes"] == (nlist + 1) * 8 + n * (M + 4)
        for k in sorted({1, 10, 257, min(n, 2048), min(n + 99, 2048)}):
            what = "%s %s n=%d top-%d" % (name, handle, n, k)
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, [ne.topk(alld[u], k) for u in use], what)
            if k <= n:
                assert same(got, idx.query_batch(qs, k)), what + ": differs from query_batch on this handle"
        if name == "overflow" and k > n:
            assert np.isposinf(got[1][got[0] >= 0]).any() and np.any(got[0] < 0), "no real id at +inf in front of the padding"


# ---- 2. list shapes -----------------------------------------------------------------------------------------------------------

def _shape_labels(n):
    """nlist = 5: list 0 empty, list 1 one node, list 2 exactly 256, list 3 257, list 4 the rest."""
    rng = np.random.default_rng(2)
    order = rng.permutation(n)
    labels = np.full(n, 4, dtype=np.int32)
    labels[order[:1]] = 1
    labels[order[1:257]] = 2
    labels[order[257:514]] = 3
    return labels


@pytest.mark.gpu
def test_list_shapes(gpu):
    c = built_class("fp32_ties")
    n = c["n"]
    labels = _shape_labels(n)
    assert np.bincount(labels, minlength=5).tolist() == [0, 1, 256, 257, n - 514]
    probes = rows([[0], [1], [2], [3], [4], [0, 1, 2, 3, 4], [3, 2], [1, 0, 2], [4, 3], [2, 2, -1, 1]], width=5)
    use, qs = queries_of(c, len(probes))
    offsets, ids = R.lists_from_labels(labels, 5, even_rule=True)
    with open_class(gpu, c) as idx:
        with gpu.IVF.from_labels(idx, labels, 5) as ivf:
            got_off, got_ids = ivf.lists()
            assert np.array_equal(got_off, offsets) and np.array_equal(got_ids, ids)
            for k in (1, 10, 256, 257, 600):
                om._rows_equal(ivf.search_probes(qs, probes, k), R.search(c["d64"], use, offsets, ids, probes, k),
                               "list shapes top-%d" % k)
        # one list that holds every node, between two empty ones
        one = np.ones(n, dtype=np.int32)
        with gpu.IVF.from_labels(idx, one, 3) as ivf:
            assert ivf.info()["max_list_len"] == n and ivf.lists()[0].tolist() == [0, 0, n, n]
            p = rows([[1], [0, 1, 2], [2, 1], [1, 1]][:4] * 2, width=3)
            use, qs = queries_of(c, len(p))
            for k in (1, 100):
                got = ivf.search_probes(qs, p, k)
                om._rows_equal(got, [ne.topk(c["d64"][u], k) for u in use], "one list of all nodes top-%d" % k)
                assert same(got, idx.query_batch(qs, k))


# ---- 3. the threshold refresh and the merge rounds --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fp32_ties", "ulp_crowd"])
def test_the_threshold_refresh(gpu, name):
    """n = 10 000 with one list of 9000: top_k 1 and 100 (a buffer of 512 keys) compact it every stride or two, 511 .. 513
    sit at the buffer of 2 x 512 and 2 x 1024, 2048 with 16 lists is 32 768 partial keys: three merge rounds."""
    n, nlist = 10000, 16
    c = built_class(name, 8, n)
    rng = np.random.default_rng(9)
    order = rng.permutation(n)
    labels = np.empty(n, dtype=np.int32)
    labels[order[:9000]] = 5
    labels[order[9000:]] = np.delete(np.arange(nlist), 5)[rng.integers(0, nlist - 1, size=1000)]
    assert np.bincount(labels, minlength=nlist)[5] == 9000
    offsets, ids = R.lists_from_labels(labels, nlist, even_rule=True)
    assert ids.max() == n                                                       # the even-N id of the last node
    rules = dict(id_base=0, n_local=n, n_total=n, even_rule=True)
    use, qs = queries_of(c, 5)
    big = rows([[5]] * 5)
    everything = np.stack([rng.permutation(nlist) for _ in range(5)]).astype(np.int32)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        for k in (1, 100, 511, 512, 513, 2048):
            om._rows_equal(ivf.search_probes(qs, big, k), R.search(c["d64"], use, offsets, ids, big, k, **rules),
                           "%s the list of 9000 top-%d" % (name, k))
        for k in (100, 2048):
            got = ivf.search_probes(qs, everything, k)
            om._rows_equal(got, R.search(c["d64"], use, offsets, ids, everything, k, **rules), "%s 16 lists top-%d" % (name, k))
            assert same(got, idx.query_batch(qs, k)), "%s 16 lists top-%d: differs from query_batch" % (name, k)


# ---- 4. padding, and the flag words -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_padding_and_probe_errors(gpu):
    import torch
    c = built_class("fp32_ties")
    n = c["n"]
    labels = _shape_labels(n)
    labels[np.flatnonzero(labels == 4)[:40]] = -1                               # forty nodes in no list
    offsets, ids = R.lists_from_labels(labels, 5, even_rule=True)
    probes = rows([[-1, -1, -1], [0, 0, -1], [0, -1, 1], [1, 1, 1], [2, 1, 0], [-1, 3, -1]], width=3)
    use, qs = queries_of(c, len(probes))
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, 5) as ivf:
        assert ivf.info()["n_unassigned"] == 40 and ivf.info()["n_assigned"] == n - 40
        for k in (10, 300):
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, R.search(c["d64"], use, offsets, ids, probes, k), "padding top-%d" % k)
            assert np.all(got[0][:2] == -1) and np.all(np.isposinf(got[1][:2]))  # all padding; an empty list alone
            assert (got[0][2] >= 0).sum() == 1 and (got[0][4] >= 0).sum() == min(k, 257)
        want = R.search(c["d64"], use, offsets, ids, probes, 10)
        # a probe >= nlist: DPQ_ERR_ARG from both forms, the device form through its flag word; the next call works
        bad = probes.copy()
        bad[3, 1] = 5
        tq = torch.from_numpy(qs).cuda()
        for call in (lambda: ivf.search_probes(qs, bad, 10),
                     lambda: ivf.search_probes_torch(tq, torch.from_numpy(bad).cuda(), 10)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == ERR_ARG
            om._rows_equal(ivf.search_probes(qs, probes, 10), want, "after a refused call")
            i, d = ivf.search_probes_torch(tq, torch.from_numpy(probes).cuda(), 10)
            om._rows_equal((i.cpu().numpy(), d.cpu().numpy()), want, "device form after a refused call")
        with pytest.raises(gpu.DpqError) as e:                                   # nprobe > nlist
            ivf.search_probes(qs, rows([[0] * 6] * len(qs)), 10)
        assert e.value.status == ERR_ARG
        with pytest.raises(gpu.DpqError) as e:                                   # no centroids
            ivf.search(qs, 2, 10)
        assert e.value.status == ERR_STATE
        with pytest.raises(gpu.DpqError) as e:
            ivf.probe(qs, 2)
        assert e.value.status == ERR_STATE
        # a label >= nlist behaves likewise; n that is not the handle's node count is refused too
        wrong = labels.copy()
        wrong[77] = 5
        for call in (lambda: gpu.IVF.from_labels(idx, wrong, 5), lambda: gpu.IVF.from_labels(idx, torch.from_numpy(wrong).cuda(), 5),
                     lambda: gpu.IVF.from_labels(idx, labels[:-1], 5)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == ERR_ARG
            with gpu.IVF.from_labels(idx, torch.from_numpy(labels).cuda(), 5) as again:
                assert np.array_equal(again.lists()[1], ids)
                om._rows_equal(again.search_probes(qs, probes, 10), want, "a structure made after a refused one")
        e = ivf.search_probes(np.zeros((0, 8), dtype=np.float32), np.zeros((0, 2), dtype=np.int32), 3)
        assert e[0].shape == (0, 3)                                              # no query is no work, and no error


# ---- 5. ids on other handle kinds ------------------------------------------------------------------------------------------------------

def _whole_index_case(c, nlist, nq, seed):
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, nlist, size=c["n"]).astype(np.int32)
    probes = np.stack([rng.permutation(nlist)[:3] for _ in range(nq)]).astype(np.int32)
    probes[1, 1] = -1
    probes[2, 2] = probes[2, 0]
    return labels, probes


@pytest.mark.gpu
def test_three_shards_take_the_same_probes_and_merge(gpu):
    c = built_class("fp32_ties", 8, 20001)
    n, nlist, nq = c["n"], 9, 6
    labels, probes = _whole_index_case(c, nlist, nq, 20)
    use, qs = queries_of(c, nq)
    offsets, ids = R.lists_from_labels(labels, nlist, even_rule=True)
    shards = [open_class(gpu, c, shard_rank=r, shard_count=3) for r in range(3)]
    try:
        bounds = [(s.info()["node_lo"], s.info()["node_hi"]) for s in shards]
        assert bounds[0][0] == 0 and bounds[2][1] == n and bounds[0][1] == bounds[1][0] and bounds[1][1] == bounds[2][0]
        for k in (10, 700):
            parts = []
            for s, (lo, hi) in zip(shards, bounds):
                with gpu.IVF.from_labels(s, labels[lo:hi], nlist) as ivf:
                    part = ivf.search_probes(qs, probes, k)
                    o, i = R.lists_from_labels(labels[lo:hi], nlist, node_lo=lo, n_total=n, even_rule=True)
                    assert np.array_equal(ivf.lists()[1], i)
                    rules = dict(id_base=lo, n_local=hi - lo, n_total=n, even_rule=True)
                    om._rows_equal(part, [R.search_row(c["d64"][u][lo:hi], o, i, probes[q], k, **rules) for q, u in enumerate(use)],
                                   "shard [%d, %d) top-%d" % (lo, hi, k))
                    parts.append(part)
            merged = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
            om._rows_equal(merged, R.search(c["d64"], use, offsets, ids, probes, k), "merged top-%d" % k)
    finally:
        for s in shards:
            s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["part", "even_n", "odd_prefix", "plain_even_n"])
def test_ids_of_parts_even_n_and_prefixes(gpu, kind):
    nlist, nq, k = 6, 6, 300
    if kind in ("even_n", "plain_even_n"):
        c = built_class("fp32_ties", 8, 4098)
        n_local, lo, n_total, opts = 4098, 0, 4098, {}
    elif kind == "part":                                                        # the part that ends an even-N index
        c = built_class("fp32_ties")
        n_local, lo = c["n"], 1000003
        n_total = lo + n_local
        opts = dict(global_offset=lo, global_n_codes=n_total)
        assert n_total % 2 == 0
    else:
        c = built_class("fp32_ties")
        n_local, lo, n_total, opts = 2731, 0, 2731, dict(num_codes=2731)
    plain = kind == "plain_even_n"
    alld = (c["d32"] if plain else c["d64"])[:, :n_local]
    labels, probes = _whole_index_case(dict(n=n_local), nlist, nq, 30)
    labels[-1] = 2                                                              # the last node is in a list every query ...
    probes[:, 0] = 2                                                            # ... probes
    use, qs = queries_of(c, nq)
    offsets, ids = R.lists_from_labels(labels, nlist, node_lo=lo, n_total=n_total, even_rule=not plain)
    assert ids.max() == (n_total if n_total % 2 == 0 and not plain else n_total - 1)
    rules = dict(id_base=lo, n_local=n_local, n_total=n_total, even_rule=not plain)
    with open_class(gpu, c, plain, **opts) as idx:
        assert (idx.info()["node_lo"], idx.info()["node_hi"]) == (lo, lo + n_local)
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            assert np.array_equal(ivf.lists()[1], ids)
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, [R.search_row(alld[u], offsets, ids, probes[q], k, **rules) for q, u in enumerate(use)], kind)
            everything = rows([np.arange(nlist)] * nq)
            with gpu.IVF.from_labels(idx, np.abs(labels), nlist) as full:       # every node labelled
                assert same(full.search_probes(qs, everything, k), idx.query_batch(qs, k)), kind + ": differs from query_batch"


# ---- 6. build from centroids ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M", [8, 16])
def test_build_from_centroids(gpu, M):
    from deltapq_amd import synth
    n, nlist, nq, k, Ds = 4097, 12, 9, 50, 4
    tree = ne.plain_tree(n, M, 256, 61)
    payload, _ = synth.encode_dtc(tree)
    codes = synth.decode_tree_codes(tree)
    cb = synth.make_codebook(M, 256, Ds, 62)
    qs = synth.make_queries(nq, M * Ds, 63)
    d64 = np.stack([C.distances(t, codes, plain=False) for t in T.l2_tables(cb, qs)])
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as idx:
        with pytest.raises(gpu.DpqError) as e:                                   # no codebook yet
            gpu.IVF.build(idx, np.zeros((nlist, M * Ds), dtype=np.float32))
        assert e.value.status == ERR_STATE
        idx.set_codebook(cb)
        recon = idx.reconstruct(R.reported_ids(0, n))
        rng = np.random.default_rng(64)
        cents = recon[rng.choice(n, size=nlist, replace=False)].copy()
        cents[1::2] += rng.normal(size=(nlist // 2, M * Ds)).astype(np.float32)
        cents[7] = cents[2]                                                      # two exact duplicates: list 7 stays empty
        labels = R.assign(recon, cents)
        assert not np.any(labels == 7) and np.any(labels == 2)
        offsets, ids = R.lists_from_labels(labels, nlist, even_rule=True)
        with gpu.IVF.build(idx, cents) as ivf:
            got_off, got_ids = ivf.lists()
            assert np.array_equal(got_off, offsets) and np.array_equal(got_ids, ids)
            inf = ivf.info()
            assert inf["has_centroids"] == 1 and inf["device_bytes"] == (nlist + 1) * 8 + n * (M + 4) + nlist * M * Ds * 4
            for nprobe in (1, 3, nlist):
                lists, cd = ivf.probe(qs, nprobe)
                want_l, want_d = R.probe(cents, qs, nprobe)
                assert np.array_equal(lists, want_l) and np.array_equal(bits(cd), bits(want_d)), "probe %d" % nprobe
                got = ivf.search(qs, nprobe, k)
                assert same(got, ivf.search_probes(qs, lists, k)), "search is not probe + search_probes"
                om._rows_equal(got, R.search(d64, np.arange(nq), offsets, ids, lists, k), "nprobe %d" % nprobe)
                import torch
                i, d = ivf.search_torch(torch.from_numpy(qs).cuda(), nprobe, k)
                assert same((i.cpu().numpy(), d.cpu().numpy()), got), "the device form differs"
            assert same(ivf.search(qs, nlist, k), idx.query_batch(qs, k))
            with gpu.IVF.from_labels(idx, labels, nlist, centroids=cents) as other:
                assert other.info()["has_centroids"] == 1
                for nprobe in (1, 3):
                    assert same(other.search(qs, nprobe, k), ivf.search(qs, nprobe, k)), "from_labels + set_centroids differs"
            with pytest.raises(gpu.DpqError) as e:                               # another number of centroids
                ivf.set_centroids(cents[:5])
            assert e.value.status == ERR_ARG


@pytest.mark.gpu
def test_the_decode_in_more_than_one_tile(gpu, monkeypatch):
    """The code gather and the assignment walk the handle in tiles of decoded segments (4 Mi nodes).  A developer
    process may shrink the tile: with tiles of two segments over 4097 nodes the lists, their codes (through the answers)
    and the labels by centroids are those of the one-tile run."""
    c = built_class("fp32_ties")
    n, nlist, k = c["n"], 7, 300
    use, qs = queries_of(c, 5)
    rng = np.random.default_rng(77)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    everything = rows([np.arange(nlist)] * 5)
    cents = (rng.normal(size=(nlist, 8)) * 50.0).astype(np.float32)
    with open_class(gpu, c) as idx:
        with gpu.IVF.build(idx, cents) as one_tile:
            want_lists = one_tile.lists()
        monkeypatch.setenv("DPQ_DEV", "1")
        monkeypatch.setenv("DPQ_IVF_TILE_NODES", "600")
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            got = ivf.search_probes(qs, everything, k)
            om._rows_equal(got, [ne.topk(c["d64"][u], k) for u in use], "tiled gather")
        with gpu.IVF.build(idx, cents) as tiled:
            got_lists = tiled.lists()
            assert np.array_equal(got_lists[0], want_lists[0]) and np.array_equal(got_lists[1], want_lists[1])
            om._rows_equal(tiled.search_probes(qs, everything, k), [ne.topk(c["d64"][u], k) for u in use], "tiled assignment")
        recon = idx.reconstruct(R.reported_ids(0, n))
        assert np.array_equal(R.lists_from_labels(R.assign(recon, cents), nlist)[1], got_lists[1])


# ---- 7. the state left behind ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_state_left_behind(gpu):
    import torch
    c = built_class("fp32_ties")
    n, nq, k, nlist = c["n"], 65, 10, 8
    use, qs = queries_of(c, nq)
    other = (use + 1) % len(c["queries"])                                       # the IVF calls ask about ANOTHER query
    qo = np.ascontiguousarray(c["queries"][other])
    rng = np.random.default_rng(41)
    labels_a = rng.integers(0, nlist, size=n).astype(np.int32)
    labels_b = rng.integers(-1, 3, size=n).astype(np.int32)
    probes_a = rng.integers(-1, nlist, size=(nq, 4)).astype(np.int32)
    probes_b = rng.integers(-1, 3, size=(nq, 2)).astype(np.int32)
    lists_a = R.lists_from_labels(labels_a, nlist)
    lists_b = R.lists_from_labels(labels_b, 3)
    want_a = R.search(c["d64"], other, *lists_a, probes_a, k)
    want_b = R.search(c["d64"], other, *lists_b, probes_b, k)
    with open_class(gpu, c, batch_decode=1) as idx:
        first = idx.query_batch(qs, k)
        om._rows_equal(first, [ne.topk(c["d64"][u], k) for u in use], "query_batch, first")
        with gpu.IVF.from_labels(idx, labels_a, nlist) as a, gpu.IVF.from_labels(idx, labels_b, 3) as b:
            assert same(idx.query_batch(qs, k), first), "query_batch changed after the constructions"
            host_a = a.search_probes(qo, probes_a, k)
            om._rows_equal(host_a, want_a, "structure a")
            om._rows_equal(b.search_probes(qo, probes_b, k), want_b, "structure b")
            om._rows_equal(a.search_probes(qo, probes_a, k), want_a, "structure a, after b")
            assert same(idx.query_batch(qs, k), first), "query_batch changed after IVF calls"
            side = torch.cuda.Stream()
            tq, tp = torch.from_numpy(qo).cuda(), torch.from_numpy(probes_a).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                i, d = a.search_probes_torch(tq, tp, k)
                with gpu.IVF.from_labels(idx, torch.from_numpy(labels_b).cuda(), 3) as b2:
                    assert np.array_equal(b2.lists()[1], lists_b[1])
            assert same((i.cpu().numpy(), d.cpu().numpy()), host_a), "the torch form on a side stream differs from the host form"
            # the coarse step on the side stream too, in the structure's own key and state workspace
            cents = rng.normal(size=(nlist, 8)).astype(np.float32) * 100.0
            a.set_centroids(cents)
            lists, _ = a.probe(qo, 3)
            assert np.array_equal(lists, R.probe(cents, qo, 3)[0])
            host_s = a.search(qo, 3, k)
            om._rows_equal(host_s, R.search(c["d64"], other, *lists_a, lists, k), "search by centroids")
            with torch.cuda.stream(side):
                i, d = a.search_torch(tq, 3, k)
            assert same((i.cpu().numpy(), d.cpu().numpy()), host_s), "search_torch on a side stream differs from the host form"
            assert same(idx.query_batch(qs, k), first), "query_batch changed after the torch forms"


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_cli_recall_with_ivf(gpu, tmp_path):
    """With -nprobe = the number of centroids the IVF line reports the exhaustive line's recall."""
    from deltapq_amd import synth
    d, n, nq, k, nlist = str(tmp_path), 2000, 12, 10, 8
    base = synth.make_clustered_vectors(n, 128, seed=91, n_clusters=60, centre_seed=90)
    qs = synth.make_clustered_vectors(nq, 128, seed=92, n_clusters=60, centre_seed=90)
    for name, v in (("learn", base), ("base", base), ("query", qs)):
        synth.write_fvecs(os.path.join(d, name + ".fvecs"), v)
    cents = os.path.join(d, "centroids.fvecs")
    synth.write_fvecs(cents, base[:nlist])
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    recall = ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-ivf", cents]
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)], recall + ["-nprobe", str(nlist)]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr    # a failed step ends the chain
    plain = re.search(r"^recall@%d = ([0-9.]+)$" % k, r.stdout, re.M)
    ivf = re.search(r"^ivf recall@%d = ([0-9.]+) \(nlist %d, nprobe %d\)$" % (k, nlist, nlist), r.stdout, re.M)
    assert plain and ivf, r.stdout
    assert ivf.group(1) == plain.group(1) and float(plain.group(1)) > 0.2
    r = subprocess.run(common + recall + ["-nprobe", str(nlist + 1)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-nprobe" in r.stdout
    for extra in (["-refine", "100"], ["-opq"]):
        r = subprocess.run(common + recall + ["-nprobe", "2"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "cannot be combined" in r.stdout, extra
