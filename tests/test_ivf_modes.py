"""IVF search with a filter, the caller's tables, the inner product and a radius (dpq_ivf_search*_filtered, *_tables, *_ip,
dpq_ivf_probe_ip, dpq_ivf_range_search*).

GPU: strictly (ids and distance bits, every query) against the restatement of tests/_ivf_modes_restatement.py over the
exact-rational reference of tests/_numeric_edges.py, and against the exhaustive calls on the same handle: list lengths
around the stride of 256 and the buffer refresh, ranks carried over several strides of the emit pass, filters that leave
nothing, one node less than top_k, single bits at word edges of a shard, the even-N bit, the slices of the range pool,
the flag words, the state a call leaves behind, the CLI.  CPU: the symbols, the hand case, the argument checks a fake
handle can reach.  Nothing is skipped and no case is exempt.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _ivf_modes_restatement as MR
import _ivf_restatement as R
import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
ERR_ARG, ERR_STATE = -1, -7
SYMBOLS = ("dpq_ivf_search_filtered", "dpq_ivf_search_device_filtered", "dpq_ivf_search_probes_filtered",
           "dpq_ivf_search_probes_device_filtered", "dpq_ivf_search_probes_tables", "dpq_ivf_search_probes_device_tables",
           "dpq_ivf_probe_ip", "dpq_ivf_search_ip", "dpq_ivf_search_device_ip", "dpq_ivf_search_probes_ip",
           "dpq_ivf_search_probes_device_ip", "dpq_ivf_range_search", "dpq_ivf_range_search_probes")
NLIST = 8
LENGTHS = (0, 1, 255, 256, 257, 513, 1500)       # lists 0 .. 6; list 7 takes the rest but the unassigned nodes
UNASSIGNED = 40
KS = (1, 10, 256, 257, 2048)
HANDLES = {"dtc_m8": (8, False), "dtc_m16": (16, False), "plain_m8": (8, True), "plain_m16": (16, True)}
CLASSES = ("ulp_crowd", "fp32_ties", "overflow")
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
    return all(np.array_equal(x, y) if x.dtype.kind == "i" else np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)) \
        and len(a) == len(b)


def open_class(api, c, plain=False, codebook=True, **opts):
    if plain:
        idx = api.DeltaPQIndex.open_plain(c["codes"], K=c["K"], **opts)
    else:
        idx = api.DeltaPQIndex.open_memory(c["payload"], c["n"], c["M"], c["K"], **opts)
    return idx.set_codebook(c["cb"]) if codebook else idx


def queries_of(c, nq):
    use = np.arange(nq) % len(c["queries"])
    return use, np.ascontiguousarray(c["queries"][use])


def rows(lists, width=None, fill=-1):
    width = max(1, max(len(l) for l in lists)) if width is None else width
    out = np.full((len(lists), width), fill, dtype=np.int32)
    for q, l in enumerate(lists):
        out[q, :len(l)] = l
    return out


def shape_labels(n, seed=3):
    """nlist = 8 with lengths 0, 1, 255, 256, 257, 513, 1500 and the rest; forty nodes in no list."""
    order = np.random.default_rng(seed).permutation(n)
    labels = np.full(n, 7, dtype=np.int32)
    at = 0
    for l, length in enumerate(LENGTHS):
        labels[order[at:at + length]] = l
        at += length
    labels[order[at:at + UNASSIGNED]] = -1
    return labels


# padding, a repeat, single lists, every list: across the stride of 256 and, for the long lists, several strides
PROBES = rows([[6], [5, -1, 4], [3, 3, 2], [1, 0], [-1, -1], [7, 6, 5, 4, 3, 2, 1, 0], [2], [4, 6, -1, 6]], width=NLIST)


def id_rules(n, plain, lo=0, n_total=None):
    return dict(id_base=lo, n_local=n, n_total=lo + n if n_total is None else n_total, even_rule=not plain)


def masks_for(n_ids, offsets, ids, k, seed=5):
    """name -> bool mask over reported ids (None: a filter that allows everything is made from an all-true mask)."""
    rng = np.random.default_rng(seed + k)
    every_third = np.zeros(n_ids, dtype=bool)
    every_third[::3] = True
    one_list = np.zeros(n_ids, dtype=bool)                 # list 4's ids only: rows that probe other lists are all padding
    one_list[ids[offsets[4]:offsets[5]]] = True
    short = np.zeros(n_ids, dtype=bool)                    # top_k - 1 nodes of the union of every list
    short[rng.choice(ids, size=min(k - 1, len(ids)), replace=False)] = True
    hundred = np.ones(100, dtype=bool)                     # n_bits = 100: ids from 100 on are not allowed
    return {"all": np.ones(n_ids, dtype=bool), "none": np.zeros(n_ids, dtype=bool), "every third": every_third,
            "one list": one_list, "top_k - 1": short, "n_bits = 100": hundred}


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in bound and hasattr(lib, name), name + " is not bound"


def test_the_hand_case():
    """N = 6 (even, DTC), labels [0, 1, 0, -1, 1, 0]: list 0 holds ids [0, 2, 6] (node 5 is reported as 6), list 1 [1, 4].
    Distances by position [5, 4, 3, 0, 1, 2]."""
    offsets, ids = R.lists_from_labels([0, 1, 0, -1, 1, 0], 2, even_rule=True)
    d = np.array([5, 4, 3, 0, 1, 2], dtype=np.float32)
    rules = dict(id_base=0, n_local=6, n_total=6, even_rule=True)
    bit6 = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)       # bit 6 set, bit 5 clear: node 5, reported as 6, stays
    bit5 = np.array([1, 1, 1, 1, 1, 1, 0], dtype=bool)       # bit 5 set, bit 6 clear: node 5 goes; bit 5 governs nothing
    assert MR.eligible_ids(bit6, 6, **rules).tolist() == [0, 1, 2, 3, 4, 6]
    assert MR.eligible_ids(bit5, 6, **rules).tolist() == [0, 1, 2, 3, 4]
    i, dd = MR.search_row(d, offsets, ids, [0, 1], 2, bit6, **rules)
    assert i.tolist() == [4, 6] and dd.tolist() == [1.0, 2.0]
    i, dd = MR.search_row(d, offsets, ids, [0, 1], 2, bit5, **rules)
    assert i.tolist() == [4, 2] and dd.tolist() == [1.0, 3.0]
    i, dd = MR.search_row(d, offsets, ids, [0, 0], 3, bit5, **rules)
    assert i.tolist() == [2, 0, -1] and dd[:2].tolist() == [3.0, 5.0] and np.isposinf(dd[2])
    i, dd = MR.search_row(d, offsets, ids, [1, -1], 2, np.array([1], dtype=bool), **rules)    # n_bits = 1: nothing of list 1
    assert i.tolist() == [-1, -1] and np.all(np.isposinf(dd))
    # a plain handle of the same six nodes: no renaming, bit 5 is node 5
    po, pi = R.lists_from_labels([0, 1, 0, -1, 1, 0], 2, even_rule=False)
    plain = dict(id_base=0, n_local=6, n_total=6, even_rule=False)
    assert MR.search_row(d, po, pi, [0], 1, bit5, **plain)[0].tolist() == [5]
    assert MR.search_row(d, po, pi, [0], 1, bit6, **plain)[0].tolist() == [2]
    # range: strict, by (distance, id); +inf takes everything eligible, 0 and negative radii nothing
    assert MR.range_row(d, offsets, ids, [0, 1], 3.0, None, **rules)[0].tolist() == [4, 6]
    assert MR.range_row(d, offsets, ids, [0, 1], np.inf, bit5, **rules)[0].tolist() == [4, 2, 1, 0]
    assert MR.range_row(d, offsets, ids, [0, 1], 0.0, None, **rules)[0].tolist() == []
    assert MR.range_row(d, offsets, ids, [0, 1], -1.0, None, **rules)[0].tolist() == []
    # inner-product coarse step: score descending, the lower list at a tie, a zero vector in between
    cents = np.array([[1, 0], [2, 0], [0, 0], [2, 0], [-1, 0]], dtype=np.float32)
    lists, scores = MR.probe_ip(cents, [[1.0, 0.0]], 5)
    assert lists[0].tolist() == [1, 3, 0, 2, 4] and scores[0].tolist() == [2.0, 2.0, 1.0, 0.0, -1.0]


def test_argument_errors_need_no_device(lib):
    """NULL pointers, a NULL filter in the _filtered forms, the bounds of top_k, nprobe and nq, and a NaN radius are
    refused before the handle is looked at (the handle below is never dereferenced) and before a device is asked for.
    (A foreign filter, a bad table entry in the host form and nq == 0 need a real structure: the GPU tests below.)"""
    buf = np.zeros(64, dtype=np.float32)
    ib = np.zeros(64, dtype=np.int32)
    p, ip, h, f = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(ib.ctypes.data), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x3000)
    # (fn, takes probes, takes a trailing stream, extra outputs)
    forms = ((lib.dpq_ivf_search_filtered, False, (), ()), (lib.dpq_ivf_search_device_filtered, False, (None,), ()),
             (lib.dpq_ivf_search_probes_filtered, True, (), ()), (lib.dpq_ivf_search_probes_device_filtered, True, (None,), ()),
             (lib.dpq_ivf_search_probes_tables, True, (), ()), (lib.dpq_ivf_search_probes_device_tables, True, (None,), ()),
             (lib.dpq_ivf_search_ip, False, (), (None, None)), (lib.dpq_ivf_search_device_ip, False, (None,), (None, None)),
             (lib.dpq_ivf_search_probes_ip, True, (), (None, None)),
             (lib.dpq_ivf_search_probes_device_ip, True, (None,), (None, None)))
    for fn, with_probes, tail, extra in forms:
        def call(v=h, flt=f, q=p, nq=1, pr=ip, nprobe=2, k=2, oi=ip, od=p):
            mid = (pr, nprobe) if with_probes else (nprobe,)
            return fn(v, flt, q, nq, *mid, k, oi, od, *extra, *tail)
        name = fn.__name__
        assert call(v=None) == ERR_ARG, name
        assert call(q=None) == ERR_ARG, name
        assert call(oi=None) == ERR_ARG, name
        assert call(od=None) == ERR_ARG, name
        assert call(nq=-1) == ERR_ARG, name
        assert call(k=0) == ERR_ARG and call(k=2049) == ERR_ARG, name
        assert call(nprobe=0) == ERR_ARG and call(nprobe=1025) == ERR_ARG, name
        if with_probes:
            assert call(pr=None) == ERR_ARG, name
        if "filtered" in name:
            assert call(flt=None) == ERR_ARG and b"filter is NULL" in lib.dpq_last_error(), name
    assert lib.dpq_ivf_probe_ip(None, p, 1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe_ip(h, None, 1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe_ip(h, p, 1, 2, None, p) == ERR_ARG
    assert lib.dpq_ivf_probe_ip(h, p, -1, 2, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe_ip(h, p, 1, 0, ip, p) == ERR_ARG
    assert lib.dpq_ivf_probe_ip(h, p, 1, 1025, ip, p) == ERR_ARG
    assert b"dpq_ivf_probe_ip" in lib.dpq_last_error()
    out = ctypes.c_void_p(0x2000)
    nan = np.array([1.0, np.nan], dtype=np.float32)
    r = ctypes.c_void_p(nan.ctypes.data)
    assert lib.dpq_ivf_range_search(h, None, p, 1, 2, r, None) == ERR_ARG
    assert lib.dpq_ivf_range_search(None, None, p, 1, 2, r, out) == ERR_ARG and out.value is None     # *out is cleared
    assert lib.dpq_ivf_range_search(h, None, None, 1, 2, r, out) == ERR_ARG
    assert lib.dpq_ivf_range_search(h, None, p, 1, 2, None, out) == ERR_ARG
    assert lib.dpq_ivf_range_search(h, None, p, -1, 2, r, out) == ERR_ARG
    assert lib.dpq_ivf_range_search(h, None, p, 1, 0, r, out) == ERR_ARG
    assert lib.dpq_ivf_range_search(h, None, p, 1, 1025, r, out) == ERR_ARG
    assert lib.dpq_ivf_range_search(h, None, p, 2, 2, r, out) == ERR_ARG and b"NaN" in lib.dpq_last_error()
    assert lib.dpq_ivf_range_search_probes(h, None, p, 1, None, 2, r, out) == ERR_ARG
    assert lib.dpq_ivf_range_search_probes(h, None, p, 2, ip, 2, r, out) == ERR_ARG and b"NaN" in lib.dpq_last_error()
    assert lib.dpq_ivf_range_search_probes(h, None, p, 1, ip, 1025, r, out) == ERR_ARG


# ---- 1. the filtered scan over the list shapes ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", CLASSES)
def test_filtered_search_over_the_list_shapes(gpu, name, handle):
    M, plain = HANDLES[handle]
    c = built_class(name, M)
    n = c["n"]
    alld = c["d32"] if plain else c["d64"]
    labels = shape_labels(n)
    assert np.bincount(labels[labels >= 0], minlength=NLIST).tolist() == list(LENGTHS) + [n - sum(LENGTHS) - UNASSIGNED]
    rules = id_rules(n, plain)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=not plain)
    use, qs = queries_of(c, len(PROBES))
    with open_class(gpu, c, plain) as idx, gpu.IVF.from_labels(idx, labels, NLIST) as ivf:
        assert np.array_equal(ivf.lists()[1], ids)
        for k in KS:
            for mname, mask in masks_for(n + 1, offsets, ids, k).items():
                what = "%s %s top-%d filter '%s'" % (name, handle, k, mname)
                with gpu.IdFilter.from_mask(idx, mask) as f:
                    got = ivf.search_probes(qs, PROBES, k, id_filter=f)
                want = MR.search(alld, use, offsets, ids, PROBES, k, mask, **rules)
                om._rows_equal(got, want, what)
                if mname == "all":
                    assert same(got, ivf.search_probes(qs, PROBES, k)), what + ": differs from the unfiltered search"
                if mname == "none":
                    assert np.all(got[0] == -1) and np.all(np.isposinf(got[1])), what
                if mname == "one list":                                       # list 4 is allowed, lists 6 and 2 are probed
                    assert np.all(got[0][0] == -1) and np.all(got[0][6] == -1) and np.any(got[0][1] >= 0), what
                if mname == "top_k - 1":
                    assert (got[0][5] >= 0).sum() == min(k - 1, len(ids)) and got[0][5][-1] == -1, what


# ---- 2. equality with the exhaustive calls ----------------------------------------------------------------------------------------

def _ip_or_error(gpu, call):
    try:
        return call(), None
    except gpu.DpqError as e:
        return None, e.status


@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", CLASSES)
def test_every_list_probed_is_the_exhaustive_call(gpu, name, handle):
    """Every node labelled and every list probed: each new call is the exhaustive call of the same handle, bit for bit."""
    M, plain = HANDLES[handle]
    c = built_class(name, M)
    n, nq, k = c["n"], 6, 100
    use, qs = queries_of(c, nq)
    rng = np.random.default_rng(11 + M)
    labels = rng.integers(0, NLIST, size=n).astype(np.int32)
    everything = np.stack([rng.permutation(NLIST) for _ in range(nq)]).astype(np.int32)
    cents = rng.normal(size=(NLIST, M)).astype(np.float32)
    mask = rng.random(n + 1) < 0.3
    tables = np.stack([ne.np_table(c["tables"][u]) for u in use])
    alld = c["d32"] if plain else c["d64"]
    with open_class(gpu, c, plain) as idx, gpu.IVF.from_labels(idx, labels, NLIST, centroids=cents) as ivf, \
            gpu.IdFilter.from_mask(idx, mask) as f:
        what = "%s %s" % (name, handle)
        assert same(ivf.search(qs, NLIST, k, id_filter=f), idx.query_batch_filtered(qs, k, f)), what + ": filtered"
        assert same(ivf.search_probes_tables(tables, everything, k), idx.query_batch_tables(tables, k)), what + ": tables"
        assert same(ivf.search_probes_tables(tables, everything, k, id_filter=f), idx.query_batch_tables(tables, k, id_filter=f)), \
            what + ": tables under a filter"
        for flt in (None, f):
            want, status = _ip_or_error(gpu, lambda: idx.query_batch_ip(qs, k, id_filter=flt))
            got, got_status = _ip_or_error(gpu, lambda: ivf.search_probes_ip(qs, everything, k, id_filter=flt))
            assert status == got_status, what + ": inner product: one call is refused and the other is not"
            if want is not None:
                assert same(got, want), what + ": inner product (ids, scores, gaps, bias)"
                assert same(ivf.search_ip(qs, NLIST, k, id_filter=flt), want), what + ": inner product by centroids"
        radii = np.array([np.sort(alld[u])[n // 2] for u in use], dtype=np.float32)
        radii[0], radii[1] = np.inf, 0.0
        got = ivf.range_search(qs, NLIST, radii)
        want = idx.range_search(qs, radii)
        assert same(got, want), what + ": range"
        om._range_equal(got, [ne.range_list(alld[u], radii[q]) for q, u in enumerate(use)], what + ": range")


# ---- 3. tables and inner product against the restatement --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
def test_tables_and_inner_product_over_the_list_shapes(gpu, handle):
    import torch
    M, plain = HANDLES[handle]
    c = built_class("fp32_ties", M)
    n = c["n"]
    labels = shape_labels(n)
    rules = id_rules(n, plain)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=not plain)
    use, qs = queries_of(c, len(PROBES))
    rng = np.random.default_rng(21)
    tables = rng.integers(0, 50, size=(len(PROBES), M, 256)).astype(np.float32)
    tables[0, 0, :7] = np.inf
    tables[1, 1, 3] = -0.0                                                       # read as +0.0
    mask = rng.random(n + 1) < 0.5
    with open_class(gpu, c, plain, codebook=False) as idx, gpu.IVF.from_labels(idx, labels, NLIST) as ivf, \
            gpu.IdFilter.from_mask(idx, mask) as f:
        for k in (10, 257):                                                      # before dpq_set_codebook
            for flt, m in ((None, None), (f, mask)):
                got = ivf.search_probes_tables(tables, PROBES, k, id_filter=flt)
                om._rows_equal(got, MR.search_tables(tables, c["codes"], plain, offsets, ids, PROBES, k, m, **rules),
                               "%s tables top-%d %s" % (handle, k, "filtered" if m is not None else ""))
                ti, td = ivf.search_probes_tables_torch(torch.from_numpy(tables).cuda(), torch.from_numpy(PROBES).cuda(), k,
                                                        id_filter=flt)
                assert same((ti.cpu().numpy(), td.cpu().numpy()), got), "the device form of the tables search differs"
        with pytest.raises(gpu.DpqError) as e:                                   # the query forms need the codebook
            ivf.search_probes_ip(qs, PROBES, 10)
        assert e.value.status == ERR_STATE
        idx.set_codebook(c["cb"])
        for k in (10, 257):
            for flt, m in ((None, None), (f, mask)):
                got = ivf.search_probes_ip(qs, PROBES, k, id_filter=flt)
                want = MR.search_ip(c["cb"], qs, c["codes"], plain, offsets, ids, PROBES, k, m, **rules)
                assert same(got, want), "%s inner product top-%d" % (handle, k)
                tq, tp = torch.from_numpy(qs).cuda(), torch.from_numpy(PROBES).cuda()
                gaps = torch.empty((len(qs), k), dtype=torch.float32, device="cuda")
                bias = torch.empty((len(qs),), dtype=torch.float32, device="cuda")
                ti, ts = ivf.search_probes_ip_torch(tq, tp, k, id_filter=flt, out_gaps=gaps, out_bias=bias)
                assert same((ti.cpu().numpy(), ts.cpu().numpy(), gaps.cpu().numpy(), bias.cpu().numpy()), got)
                ti, ts = ivf.search_probes_ip_torch(tq, tp, k, id_filter=flt)   # without gaps and bias
                assert same((ti.cpu().numpy(), ts.cpu().numpy()), got[:2])


@pytest.mark.gpu
def test_the_inner_product_coarse_step(gpu):
    """Centroids with two exact duplicates (the tie goes to the lower list) and one zero vector."""
    import torch
    c = built_class("fp32_ties", 8)
    n, k = c["n"], 20
    rng = np.random.default_rng(31)
    labels = rng.integers(0, NLIST, size=n).astype(np.int32)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=True)
    cents = rng.normal(size=(NLIST, 8)).astype(np.float32) * 30.0
    cents[6] = cents[2]
    cents[4] = 0.0
    qs = np.ascontiguousarray(np.concatenate([c["queries"], rng.normal(size=(5, 8)).astype(np.float32) * 100.0]))
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, NLIST, centroids=cents) as ivf:
        for nprobe in (1, 3, NLIST):
            lists, scores = ivf.probe_ip(qs, nprobe)
            want_l, want_s = MR.probe_ip(cents, qs, nprobe)
            assert np.array_equal(lists, want_l) and np.array_equal(bits(scores), bits(want_s)), "probe_ip %d" % nprobe
            got = ivf.search_ip(qs, nprobe, k)
            assert same(got, ivf.search_probes_ip(qs, lists, k)), "search_ip is not probe_ip + search_probes_ip"
            assert same(got, MR.search_ip(c["cb"], qs, c["codes"], False, offsets, ids, lists, k, **id_rules(n, False)))
            ti, ts = ivf.search_ip_torch(torch.from_numpy(qs).cuda(), nprobe, k)
            assert same((ti.cpu().numpy(), ts.cpu().numpy()), got[:2]), "the device form differs"
        full = ivf.probe_ip(qs, NLIST)[0]
        for row in full:                                                         # the duplicates tie: list 2 before list 6
            assert list(row).index(2) < list(row).index(6)
        assert full[0].tolist() == list(range(NLIST))                            # the all-zero query: every score is +0.0


# ---- 4. the even-N bit, and single bits on a shard -----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_even_n_bit(gpu):
    """n = 4098 (DTC): the last node, reported as 4098, is in a probed list.  Bit N alone keeps it; bit N - 1 alone keeps
    nothing."""
    c = built_class("fp32_ties", 8, 4098)
    n = c["n"]
    labels = shape_labels(n)
    labels[-1] = 4
    rules = id_rules(n, False)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=True)
    assert ids.max() == n
    probes = rows([[4], [4, 3], [7, 4, -1]])
    use, qs = queries_of(c, len(probes))
    radii = np.full(len(qs), np.inf, dtype=np.float32)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, NLIST) as ivf:
        for bit, found in ((n, [n]), (n - 1, [])):
            mask = np.zeros(n + 1, dtype=bool)
            mask[bit] = True
            with gpu.IdFilter.from_mask(idx, mask) as f:
                got = ivf.search_probes(qs, probes, 3, id_filter=f)
                om._rows_equal(got, MR.search(c["d64"], use, offsets, ids, probes, 3, mask, **rules), "bit %d" % bit)
                assert all(r[r >= 0].tolist() == found for r in got[0]), "bit %d" % bit
                assert same(got, idx.query_batch_filtered(qs, 3, f)), "bit %d: differs from query_batch_filtered" % bit
                rng_got = ivf.range_search_probes(qs, probes, radii, id_filter=f)
                om._range_equal(rng_got, MR.range_search(c["d64"], use, offsets, ids, probes, radii, mask, **rules), "range, bit %d" % bit)
                assert rng_got[1].tolist() == found * len(qs)


@pytest.mark.gpu
def test_single_bits_on_a_shard(gpu):
    """The second of three shards (id_base > 0): a filter of one global id whose local node is 31, 32, 63 or 64 -- the
    edges of the bitmap's words."""
    c = built_class("fp32_ties", 8, 20001)
    n_total = c["n"]
    nq, k = 4, 5
    use, qs = queries_of(c, nq)
    everything = rows([np.arange(NLIST)] * nq)
    with open_class(gpu, c, shard_rank=1, shard_count=3) as idx:
        lo, hi = idx.info()["node_lo"], idx.info()["node_hi"]
        assert lo > 0 and hi < n_total
        n = hi - lo
        labels = np.random.default_rng(51).integers(0, NLIST, size=n).astype(np.int32)
        rules = id_rules(n, False, lo=lo, n_total=n_total)
        offsets, ids = R.lists_from_labels(labels, NLIST, node_lo=lo, n_total=n_total, even_rule=True)
        d = c["d64"][:, lo:hi]
        radii = np.full(nq, np.inf, dtype=np.float32)
        with gpu.IVF.from_labels(idx, labels, NLIST) as ivf:
            assert np.array_equal(ivf.lists()[1], ids)
            for local in (31, 32, 63, 64):
                mask = np.zeros(n_total + 1, dtype=bool)
                mask[lo + local] = True
                with gpu.IdFilter.from_mask(idx, mask) as f:
                    got = ivf.search_probes(qs, everything, k, id_filter=f)
                    om._rows_equal(got, MR.search(d, use, offsets, ids, everything, k, mask, **rules), "local %d" % local)
                    assert np.all(got[0][:, 0] == lo + local) and np.all(got[0][:, 1:] == -1)
                    assert same(got, idx.query_batch_filtered(qs, k, f))
                    lims, ri, _ = ivf.range_search_probes(qs, everything, radii, id_filter=f)
                    assert lims.tolist() == list(range(nq + 1)) and np.all(ri == lo + local)
            mask = np.random.default_rng(52).random(n_total + 1) < 0.4           # global ids, most of them other shards'
            with gpu.IdFilter.from_mask(idx, mask) as f:
                om._rows_equal(ivf.search_probes(qs, everything[:, :3], 300, id_filter=f),
                               MR.search(d, use, offsets, ids, everything[:, :3], 300, mask, **rules), "a random mask on the shard")


# ---- 5. range search ----------------------------------------------------------------------------------------------------------------------

def _radii(alld, use, offsets, ids, probes, mask, rules):
    """Per query: a negative radius, 0, the smallest distance of the (eligible) union, the next float above it, the
    median, +inf -- in turn."""
    out = np.zeros(len(use), dtype=np.float32)
    for q, u in enumerate(use):
        _, d = MR.range_row(alld[u], offsets, ids, probes[q], np.inf, mask, **rules)
        kind = q % 6
        if kind == 0:
            out[q] = -1.0
        elif kind == 1 or len(d) == 0:
            out[q] = 0.0
        elif kind == 2:
            out[q] = d[0]
        elif kind == 3:
            out[q] = np.nextafter(d[0], np.float32(np.inf))
        elif kind == 4:
            out[q] = d[len(d) // 2]
        else:
            out[q] = np.inf
    return out


RANGE_PROBES = rows([[6], [6, 5], [6, 5, 4], [7, 6, 5, 4, 3, 2, 1, 0], [5, 5, 2, -1], [7, 6, 5, 4, 3, 2, 1, 0],
                     [-1, -1], [0, 1], [3], [2, 4], [7, 6], [6, 7, 1]], width=NLIST)


@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", CLASSES)
def test_range_search_over_the_list_shapes(gpu, name, handle):
    M, plain = HANDLES[handle]
    c = built_class(name, M)
    n = c["n"]
    alld = c["d32"] if plain else c["d64"]
    labels = shape_labels(n)
    rules = id_rules(n, plain)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=not plain)
    use, qs = queries_of(c, len(RANGE_PROBES))
    third = np.zeros(n + 1, dtype=bool)
    third[::3] = True
    with open_class(gpu, c, plain) as idx, gpu.IVF.from_labels(idx, labels, NLIST) as ivf, gpu.IdFilter.from_mask(idx, third) as f:
        for flt, mask in ((None, None), (f, third)):
            radii = _radii(alld, use, offsets, ids, RANGE_PROBES, mask, rules)
            want = MR.range_search(alld, use, offsets, ids, RANGE_PROBES, radii, mask, **rules)
            what = "%s %s range%s" % (name, handle, " under a filter" if mask is not None else "")
            assert len(want[0][0]) == 0 and len(want[1][0]) == 0 and len(want[5][0]) > 1000, what + ": the radii do not cut"
            if np.isfinite(radii[2]):                                            # strict: the nearest node itself is left out
                assert len(want[2][0]) == 0 and len(want[3][0]) >= 1, what + ": the radii do not cut"
            got = ivf.range_search_probes(qs, RANGE_PROBES, radii, id_filter=flt)
            om._range_equal(got, want, what)
            if name == "overflow":
                assert np.isposinf(got[2]).any(), what + ": no node at +inf under the radius +inf"


@pytest.mark.gpu
def test_range_search_across_the_pool(gpu, monkeypatch):
    """A developer process may shrink the pool of keys: with 3000 keys the batch below takes three groups, and the query
    that probes every list (4057 keys) alone exceeds the pool and works in buffers of the call.  The answer is the
    one-group run's."""
    c = built_class("ulp_crowd", 8)
    n = c["n"]
    labels = shape_labels(n)
    rules = id_rules(n, False)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=True)
    probes = rows([[6], [5, 4], [7, 6, 5, 4, 3, 2, 1, 0], [6, 2], [3]], width=NLIST)
    use, qs = queries_of(c, len(probes))
    radii = np.full(len(qs), np.inf, dtype=np.float32)
    want = MR.range_search(c["d64"], use, offsets, ids, probes, radii, None, **rules)
    assert [len(w[0]) for w in want] == [1500, 770, n - UNASSIGNED, 1755, 256]  # groups of 3000: {0, 1}, {2} alone, {3, 4}
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, NLIST) as ivf:
        whole = ivf.range_search_probes(qs, probes, radii)
        om._range_equal(whole, want, "one group")
        monkeypatch.setenv("DPQ_DEV", "1")
        monkeypatch.setenv("DPQ_IVF_RANGE_POOL_KEYS", "3000")
        om._range_equal(ivf.range_search_probes(qs, probes, radii), want, "three groups")
        monkeypatch.setenv("DPQ_IVF_RANGE_POOL_KEYS", "1")                       # every query on its own
        om._range_equal(ivf.range_search_probes(qs, probes, radii), want, "a group per query")
        monkeypatch.delenv("DPQ_IVF_RANGE_POOL_KEYS")
        assert same(ivf.range_search_probes(qs, probes, radii), whole)


@pytest.mark.gpu
def test_range_lists_of_shards_merge(gpu):
    from deltapq_amd import dist
    c = built_class("fp32_ties", 8, 20001)
    n, nq = c["n"], 6
    use, qs = queries_of(c, nq)
    rng = np.random.default_rng(61)
    labels = rng.integers(-1, NLIST, size=n).astype(np.int32)
    probes = np.stack([rng.permutation(NLIST)[:3] for _ in range(nq)]).astype(np.int32)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=True)
    mask = rng.random(n + 1) < 0.5
    radii = _radii(c["d64"], use, offsets, ids, probes, mask, id_rules(n, False))
    parts, tops = [], []
    for r in range(3):
        with open_class(gpu, c, shard_rank=r, shard_count=3) as s:
            lo, hi = s.info()["node_lo"], s.info()["node_hi"]
            with gpu.IVF.from_labels(s, labels[lo:hi], NLIST) as ivf, gpu.IdFilter.from_mask(s, mask) as f:
                parts.append(ivf.range_search_probes(qs, probes, radii, id_filter=f))
                tops.append(ivf.search_probes(qs, probes, 50, id_filter=f))
    om._range_equal(dist.merge_range_host(parts), MR.range_search(c["d64"], use, offsets, ids, probes, radii, mask, **id_rules(n, False)),
                    "merged range lists")
    merged = gpu.merge_topk_host(np.stack([t[0] for t in tops]), np.stack([t[1] for t in tops]))
    om._rows_equal(merged, MR.search(c["d64"], use, offsets, ids, probes, 50, mask, **id_rules(n, False)), "merged filtered top-50")


# ---- 6. device forms, flag words, argument errors on a real structure ------------------------------------------------------------

@pytest.mark.gpu
def test_device_forms_and_flag_words(gpu):
    import torch
    c = built_class("fp32_ties")
    n, k = c["n"], 10
    labels = shape_labels(n)
    rules = id_rules(n, False)
    offsets, ids = R.lists_from_labels(labels, NLIST, even_rule=True)
    use, qs = queries_of(c, len(PROBES))
    rng = np.random.default_rng(71)
    mask = rng.random(n + 1) < 0.5
    cents = rng.normal(size=(NLIST, 8)).astype(np.float32) * 50.0
    tables = rng.integers(0, 50, size=(len(PROBES), 8, 256)).astype(np.float32)
    tq, tp, tt = torch.from_numpy(qs).cuda(), torch.from_numpy(PROBES).cuda(), torch.from_numpy(tables).cuda()
    down = lambda pair: tuple(t.cpu().numpy() for t in pair)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, NLIST, centroids=cents) as ivf, \
            gpu.IdFilter.from_mask(idx, mask) as f, open_class(gpu, c) as other, gpu.IdFilter.from_mask(other, mask) as foreign:
        host = ivf.search_probes(qs, PROBES, k, id_filter=f)
        om._rows_equal(host, MR.search(c["d64"], use, offsets, ids, PROBES, k, mask, **rules), "host form")
        assert same(down(ivf.search_probes_torch(tq, tp, k, id_filter=f)), host), "search_probes_torch differs"
        by_cents = ivf.search(qs, 3, k, id_filter=f)
        assert same(by_cents, ivf.search_probes(qs, ivf.probe(qs, 3)[0], k, id_filter=f)), "search is not probe + search_probes"
        assert same(down(ivf.search_torch(tq, 3, k, id_filter=f)), by_cents), "search_torch differs"
        want_t = ivf.search_probes_tables(tables, PROBES, k, id_filter=f)
        # the flag words: a probe >= nlist and a NaN table entry return DPQ_ERR_ARG from the device forms, the next call works
        bad_p = PROBES.copy()
        bad_p[2, 1] = NLIST
        bad_t = tables.copy()
        bad_t[3, 5, 17] = np.nan
        for call in (lambda: ivf.search_probes_torch(tq, torch.from_numpy(bad_p).cuda(), k, id_filter=f),
                     lambda: ivf.search_probes_tables_torch(tt, torch.from_numpy(bad_p).cuda(), k),
                     lambda: ivf.search_probes_ip_torch(tq, torch.from_numpy(bad_p).cuda(), k),
                     lambda: ivf.search_probes_tables_torch(torch.from_numpy(bad_t).cuda(), tp, k, id_filter=f),
                     # the host forms check on the host
                     lambda: ivf.search_probes(qs, bad_p, k, id_filter=f),
                     lambda: ivf.search_probes_tables(bad_t, PROBES, k),
                     lambda: ivf.search_probes_tables(-tables - 1.0, PROBES, k),
                     lambda: ivf.range_search_probes(qs, bad_p, 1.0),
                     # a filter of another handle, in every family
                     lambda: ivf.search_probes(qs, PROBES, k, id_filter=foreign),
                     lambda: ivf.search_torch(tq, 3, k, id_filter=foreign),
                     lambda: ivf.search_probes_tables(tables, PROBES, k, id_filter=foreign),
                     lambda: ivf.search_ip(qs, 3, k, id_filter=foreign),
                     lambda: ivf.range_search(qs, 3, 1.0, id_filter=foreign),
                     # nprobe > nlist
                     lambda: ivf.search_ip(qs, NLIST + 1, k),
                     lambda: ivf.range_search(qs, NLIST + 1, 1.0),
                     lambda: ivf.probe_ip(qs, NLIST + 1)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == ERR_ARG
            assert same(down(ivf.search_probes_tables_torch(tt, tp, k, id_filter=f)), want_t), "after a refused call"
            assert same(ivf.search_probes(qs, PROBES, k, id_filter=f), host), "after a refused call"
        with pytest.raises(TypeError):
            ivf.search(qs, 3, k, id_filter=mask)                                 # not an IdFilter
        # no query is no work, and no error
        none_q, none_p = np.zeros((0, 8), dtype=np.float32), np.zeros((0, 2), dtype=np.int32)
        assert ivf.search_probes(none_q, none_p, 3, id_filter=f)[0].shape == (0, 3)
        assert ivf.search_probes_ip(none_q, none_p, 3)[0].shape == (0, 3)
        assert ivf.search_probes_tables(np.zeros((0, 8, 256), dtype=np.float32), none_p, 3)[0].shape == (0, 3)
        lims, ri, rd = ivf.range_search_probes(none_q, none_p, np.zeros(0, dtype=np.float32))
        assert lims.tolist() == [0] and len(ri) == 0 and len(rd) == 0
        # without centroids the coarse forms are DPQ_ERR_STATE
        with gpu.IVF.from_labels(idx, labels, NLIST) as bare:
            for call in (lambda: bare.search(qs, 2, k, id_filter=f), lambda: bare.search_ip(qs, 2, k),
                         lambda: bare.probe_ip(qs, 2), lambda: bare.range_search(qs, 2, 1.0)):
                with pytest.raises(gpu.DpqError) as e:
                    call()
                assert e.value.status == ERR_STATE


# ---- 7. the state left behind ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_state_left_behind(gpu):
    """query_batch and the unfiltered ivf.search give the same bits before and after every new call."""
    c = built_class("fp32_ties")
    n, nq, k = c["n"], 33, 10
    use, qs = queries_of(c, nq)
    qo = np.ascontiguousarray(c["queries"][(use + 1) % len(c["queries"])])       # the new calls ask about ANOTHER query
    rng = np.random.default_rng(81)
    labels = rng.integers(-1, NLIST, size=n).astype(np.int32)
    probes = rng.integers(-1, NLIST, size=(nq, 4)).astype(np.int32)
    cents = rng.normal(size=(NLIST, 8)).astype(np.float32) * 50.0
    tables = rng.integers(0, 50, size=(nq, 8, 256)).astype(np.float32)
    mask = rng.random(n + 1) < 0.5
    with open_class(gpu, c, batch_decode=1) as idx, gpu.IVF.from_labels(idx, labels, NLIST, centroids=cents) as ivf, \
            gpu.IdFilter.from_mask(idx, mask) as f:
        first = idx.query_batch(qs, k)
        om._rows_equal(first, [ne.topk(c["d64"][u], k) for u in use], "query_batch, first")
        plain_ivf = ivf.search(qs, 3, k)
        for name, call in (("filtered", lambda: ivf.search(qo, 3, k, id_filter=f)),
                           ("probes filtered", lambda: ivf.search_probes(qo, probes, k, id_filter=f)),
                           ("tables", lambda: ivf.search_probes_tables(tables, probes, k, id_filter=f)),
                           ("probe_ip", lambda: ivf.probe_ip(qo, 3)),
                           ("ip", lambda: ivf.search_ip(qo, 3, k)),
                           ("probes ip", lambda: ivf.search_probes_ip(qo, probes, k, id_filter=f)),
                           ("range", lambda: ivf.range_search(qo, 3, np.float32(np.inf), id_filter=f)),
                           ("range probes", lambda: ivf.range_search_probes(qo, probes, np.float32(np.inf)))):
            once = call()
            assert same(idx.query_batch(qs, k), first), "query_batch changed after " + name
            assert same(ivf.search(qs, 3, k), plain_ivf), "the unfiltered ivf.search changed after " + name
            assert same(call(), once), name + " is not repeatable"


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_cli_recall_with_ivf_under_a_filter_and_the_inner_product(gpu, tmp_path):
    """With -nprobe = the number of centroids the IVF line reports the exhaustive line's recall of the same run: under
    -filter, under -metric ip, and under both.  The refusals that remain keep their text."""
    from deltapq_amd import synth
    d, n, nq, k, nlist = str(tmp_path), 2000, 12, 10, 8
    base = synth.make_clustered_vectors(n, 128, seed=91, n_clusters=60, centre_seed=90)
    qs = synth.make_clustered_vectors(nq, 128, seed=92, n_clusters=60, centre_seed=90)
    for name, v in (("learn", base), ("base", base), ("query", qs)):
        synth.write_fvecs(os.path.join(d, name + ".fvecs"), v)
    cents = os.path.join(d, "centroids.fvecs")
    synth.write_fvecs(cents, base[:nlist])
    fpath = os.path.join(d, "third.bitmap")
    gpu.write_bitmap(fpath, *gpu.FlatIdFilter.pack_mask(np.arange(n) % 3 == 0))
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    gt = ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)]
    recall = ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-ivf", cents]
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr    # a failed step ends the chain
    for extra, exhaustive in ((["-filter", fpath], "filtered recall"), (["-metric", "ip"], "recall"),
                              (["-metric", "ip", "-filter", fpath], "filtered recall")):
        for args in (gt + extra, recall + ["-nprobe", str(nlist)] + extra):
            r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
        plain = re.search(r"^%s@%d = ([0-9.]+)$" % (exhaustive, k), r.stdout, re.M)
        ivf = re.search(r"^ivf recall@%d = ([0-9.]+) \(nlist %d, nprobe %d\)$" % (k, nlist, nlist), r.stdout, re.M)
        assert plain and ivf, r.stdout
        assert ivf.group(1) == plain.group(1) and float(plain.group(1)) > 0.2, " ".join(extra) + "\n" + r.stdout
        r = subprocess.run(common + recall + ["-nprobe", "1"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and re.search(r"^ivf recall@%d = " % k, r.stdout, re.M), r.stdout + r.stderr
    for extra in (["-refine", "100"], ["-opq"], ["-gpus", "2"]):
        r = subprocess.run(common + recall + ["-nprobe", "2"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "cannot be combined" in r.stdout, extra
