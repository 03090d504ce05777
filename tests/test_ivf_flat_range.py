"""Range search over the raw-vector IVF (include/deltapq_amd.h "IVF range search over raw vectors").  The
reference is the keys the existing restatements form for the rows of a query's probed lists -- tests/_flat_ivf_restatement.py
for L2, the binary suite's Hamming table, tests/_exact_ip_restatement.py and _exact_bytes_ip_restatement.py for inner product
-- cut by the strict rule d < r / s > t.  Every path is exact by construction: lims, ids and value bits are equal."""
import ctypes

import numpy as np
import pytest

import _exact_ip_restatement as XI
import test_ivf_flat as T
import test_ivf_flat_bits as BI
import test_ivf_flat_modes as M
from _flat_ivf_restatement import lists_from_labels, row_keys

ERR_ARG = -1
F32 = np.float32
pytestmark = pytest.mark.gpu
gpu = T.gpu
SYMBOLS = tuple("dpq_flat_ivf_range_search%s%s" % (p, k) for p in ("", "_probes") for k in ("", "_ip", "_bytes", "_ip_bytes", "_bits"))
# the fp32 scan's partial first slice, partial second slice and whole slices; the other formats at the edges their suites use
WIDTHS = [("f32", D) for D in (4, 36, 128)] + [w for w in M.IP_WIDTHS if w[0] != "f32"] + [("bits", D) for D in (1, 13, 129, 1024)]


def family(fmt, D):
    return (BI.make_case(D), BI.open_case) if fmt == "bits" else M.ip_family(fmt, D)


def keys_of(c, ip, i, row, off=0, mask=None):
    """uint64, ascending: the keys of query i over the rows of the lists its probe row names, intersected with the mask."""
    if mask is not None:
        c = M.cut_lists(c, mask)
    if not ip and "dist" not in c:
        return row_keys(c, c["qs"][i], row, off)
    r = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in dict.fromkeys(int(p) for p in row if p >= 0)] +
                       [np.zeros(0, dtype=np.int64)])
    if ip:
        return np.sort(XI.keys(M.ip_table(c)[i, r], r + off))
    return np.sort((c["dist"][i, r].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (r + off).astype(np.uint64))


def values(keys, ip):
    w = (keys >> np.uint64(32)).astype(np.uint32)
    return (XI.word(w) if ip else w).view(F32)


def bounds_of(c, ip, probes):
    """One bound per query, by q % 5: nothing passes (r <= 0 / t = +inf); beyond the best row; the middle row's value (hits
    in the near lists, none in the far ones); a row's own value (strict); everything (+inf / -inf)."""
    out = np.empty(len(probes), dtype=F32)
    for i, row in enumerate(probes):
        v = values(keys_of(c, ip, i, row), ip)
        v = v if len(v) else np.ones(1, dtype=F32)
        beyond = np.nextafter(v[0], F32(np.inf)) if ip else v[0] * F32(0.5)
        out[i] = [np.inf if ip else -(i % 2), beyond, v[len(v) // 2], v[len(v) // 3], -np.inf if ip else np.inf][i % 5]
    return out


def want(c, ip, probes, bounds, off=0, mask=None):
    lims, ids, vals = [0], [], []
    for i, row in enumerate(probes):
        k = keys_of(c, ip, i, row, off, mask)
        v = values(k, ip)
        k = k[v > bounds[i]] if ip else k[(v < bounds[i]) & (bounds[i] > 0)]
        ids.append((k & np.uint64(0xffffffff)).astype(np.uint32).view(np.int32))
        vals.append(values(k, ip))
        lims.append(lims[-1] + len(k))
    return np.array(lims, dtype=np.int64), np.concatenate(ids), np.concatenate(vals)


def same(got, exp):
    return all(np.array_equal(g, w) for g, w in zip(got[:2], exp[:2])) and np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32))


def call(ivf, ip, *args, **kw):
    return (ivf.range_search_probes_ip if ip else ivf.range_search_probes)(*args, **kw)


@pytest.mark.parametrize("fmt,D", WIDTHS)
def test_probed_lists_at_the_width_edges(gpu, fmt, D):
    """The suites' own lists (0, 1, 255, 256, 257, 1500 ... rows) and probes (-1 padding, a repeated list, up to 17 queries
    per list), the five kinds of bound in one call, at a non-zero id_offset."""
    c, open_case = family(fmt, D)
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf:
        for ip in (False, True)[:1 if fmt == "bits" else 2]:
            b = bounds_of(c, ip, c["probes"])
            exp = want(c, ip, c["probes"], b, 7)
            assert exp[0][-1] > 0 and same(call(ivf, ip, c["qs"], c["probes"], b), exp)


@pytest.mark.parametrize("every", [1, 10, 0])
@pytest.mark.parametrize("fmt", ["f32", "sq8", "u8", "bits"])
def test_under_an_id_filter(gpu, fmt, every):
    """A filter that allows everything, every tenth row, and nothing."""
    c, open_case = family(fmt, 33 if fmt != "bits" else 100)
    mask, what = np.arange(len(c["base"])) % max(every, 1) == 0, "ids"
    mask &= every > 0
    flat, ivf = open_case(gpu, c)
    with flat, ivf, M.make_filter(gpu, flat, mask, what) as filt:
        for ip in (False, True)[:1 if fmt == "bits" else 2]:
            b = bounds_of(c, ip, c["probes"])
            assert same(call(ivf, ip, c["qs"], c["probes"], b, id_filter=filt), want(c, ip, c["probes"], b, 0, mask))


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_the_answer_does_not_depend_on_the_group(gpu, monkeypatch, fmt, G):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    c, open_case = family(fmt, 33)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        for ip in (False, True):
            b = bounds_of(c, ip, c["probes"])
            assert same(call(ivf, ip, c["qs"], c["probes"], b), want(c, ip, c["probes"], b))


@pytest.mark.parametrize("pool", [2000, 40])
@pytest.mark.parametrize("fmt", ["f32", "f16", "i8", "bits"])
def test_sub_batches_and_a_pool_of_the_call(gpu, monkeypatch, fmt, pool):
    """A pool of 2000 keys: several sub-batches, whose emit launches drop the other queries' pairs; of 40: most queries
    with hits need buffers of their own."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_IVF_RANGE_POOL_KEYS", str(pool))
    c, open_case = family(fmt, 33 if fmt != "bits" else 100)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        b = bounds_of(c, False, c["probes"])
        exp = want(c, False, c["probes"], b)
        assert np.diff(exp[0]).max() > 40 and exp[0][-1] > 2 * 2000 and same(ivf.range_search_probes(c["qs"], c["probes"], b), exp)


@pytest.mark.parametrize("ip", [False, True])
def test_one_query_more_than_a_slice(gpu, ip):
    rng = np.random.default_rng(5)
    c = dict(base=rng.standard_normal((300, 4)).astype(F32), qs=rng.standard_normal((2049, 4)).astype(F32),
             labels=(np.arange(300) % 4 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 3)
    probes = np.stack([np.arange(2049) % 3, (np.arange(2049) // 3) % 3], 1).astype(np.int32)
    with gpu.FlatIndex(c["base"]) as flat, gpu.FlatIVF.from_labels(flat, c["labels"], 3) as ivf:
        b = np.full(2049, 0.5 if ip else 2.0, dtype=F32)
        exp = want(c, ip, probes, b)
        assert exp[0][-1] > exp[0][2048] > 0 and same(call(ivf, ip, c["qs"], probes, b), exp)


@pytest.mark.parametrize("fmt", ["f32", "f16", "bf16", "sq8", "sq4", "u8", "i8", "bits"])
def test_it_agrees_with_the_exhaustive_search(gpu, fmt):
    """The handle's own range_search[_ip] under a filter of the probed lists' rows, intersected with an id filter; and the
    coarse-step form is range_search_probes of probe's / probe_ip's lists."""
    c, open_case = family(fmt, 33 if fmt != "bits" else 100)
    long = {"u8": M.BY.LONG, "i8": M.BY.LONG, "bits": BI.LONG}.get(fmt, 5)
    mask = M.mask_of(c, long, "odd")
    probes = np.array([[long, 2, 7]], dtype=np.int32)
    union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf, M.make_filter(gpu, flat, mask, "odd", 7) as filt, gpu.FlatIdFilter.from_ids(flat, union + 7) as lists, \
            gpu.FlatIdFilter.from_ids(flat, union[mask[union]] + 7) as both:
        for ip in (False, True)[:1 if fmt == "bits" else 2]:
            whole, given = (flat.range_search_ip, ivf.range_search_ip) if ip else (flat.range_search, ivf.range_search)
            v = values(keys_of(c, ip, 0, probes[0]), ip)
            b = v[len(v) // 3:len(v) // 3 + 1]                                      # a row's own value, and the next one up
            for r in (b, np.nextafter(b, F32(np.inf)), np.array([-np.inf if ip else np.inf], dtype=F32)):
                assert same(call(ivf, ip, c["qs"][:1], probes, r), whole(c["qs"][:1], r, lists))
                assert same(call(ivf, ip, c["qs"][:1], probes, r, id_filter=filt), whole(c["qs"][:1], r, both))
            named = (ivf.probe_ip if ip else ivf.probe)(c["qs"], 5)[0]
            b = bounds_of(c, ip, named)
            got = given(c["qs"], 5, b, id_filter=filt)
            assert same(got, call(ivf, ip, c["qs"], named, b, id_filter=filt)) and same(got, want(c, ip, named, b, 7, mask))


def test_what_is_refused(gpu, lib):
    from deltapq_amd import _lib
    assert {n for n, _, _ in _lib.SYMBOLS} >= set(SYMBOLS) and all(hasattr(lib, n) for n in SYMBOLS)
    c = T.make_case(33)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    one = np.ones(len(c["qs"]), dtype=F32)
    flat, ivf = T.open_case(gpu, c)
    with flat, ivf, gpu.FlatIndex(c["base"]) as other, gpu.FlatIdFilter.from_mask(other, np.ones(len(c["base"]), dtype=bool)) as alien:
        nan = one.copy()
        nan[3] = np.nan
        q, res = c["qs"].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
        # a NaN bound is refused before the structure is looked at: the handle is never dereferenced
        assert lib.dpq_flat_ivf_range_search(ctypes.c_void_p(0x1000), None, q, len(one), 2, nan.ctypes.data_as(ctypes.c_void_p), res) == ERR_ARG
        assert status(lambda: ivf.range_search(c["qs"], 2, nan)) == ERR_ARG and status(lambda: ivf.range_search_probes_ip(c["qs"], c["probes"], nan)) == ERR_ARG
        assert status(lambda: ivf.range_search_probes(c["qs"], c["probes"], one, id_filter=alien)) == ERR_ARG
        assert status(lambda: ivf.range_search(c["qs"], 0, one)) == ERR_ARG and status(lambda: ivf.range_search(c["qs"], T.NLIST + 1, one)) == ERR_ARG
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert lib.dpq_flat_ivf_range_search_probes_bytes(ivf._h, None, q, len(one), ptr(c["probes"]), 4, ptr(one), res) == ERR_ARG
        lims, ids, dists = ivf.range_search(c["qs"][:0], 2, one[:0])                # nq == 0: an empty result
        assert lims.tolist() == [0] and len(ids) == 0 and len(dists) == 0
        b = bounds_of(c, False, c["probes"])                                       # the next call works
        assert same(ivf.range_search_probes(c["qs"], c["probes"], b), want(c, False, c["probes"], b))
    y = M.BY.make_case("u8", 33)
    flat, ivf = M.BY.open_case(gpu, y)
    with flat, ivf:
        r = np.ones(len(y["qs"]), dtype=F32)
        assert lib.dpq_flat_ivf_range_search_probes(ivf._h, None, ptr(y["qs"]), len(r), ptr(y["probes"]), y["probes"].shape[1], ptr(r), res) == ERR_ARG
    b = BI.make_case(100)
    flat, ivf = BI.open_case(gpu, b)
    with flat, ivf:                                                                # binary rows have no inner product
        assert status(lambda: ivf.range_search_ip(b["qs"], 2, 1.0)) == ERR_ARG
        assert status(lambda: ivf.range_search_probes_ip(b["qs"], b["probes"], 1.0)) == ERR_ARG
