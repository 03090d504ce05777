"""IVF search over raw vectors by inner product and under an id filter (include/deltapq_amd.h "IVF search over raw vectors
by inner product" and "... under an id filter").  The references are the restatements that exist: for L2
under a filter the one each kind of rows has (tests/_flat_ivf_restatement.py; the binary suite's Hamming table) over lists
cut to the eligible rows; for inner product tests/_exact_ip_restatement.py and tests/_exact_bytes_ip_restatement.py with
`allowed` = the rows of the query's probed lists, intersected with the filter.  The arithmetic is stated exactly, so there
is no tolerance: ids and value bits are equal, padding is -1 / +inf for L2 and -1 / -inf for inner product."""
import ctypes

import numpy as np
import pytest

import _exact_bytes_ip_restatement as BX
import _exact_ip_restatement as XI
import test_ivf_flat as T
import test_ivf_flat_bits as BI
import test_ivf_flat_bytes as BY
import test_ivf_flat_narrow as N
from _flat_ivf_restatement import lists_from_labels, same, search

ERR_ARG = -1
F32 = np.float32
pytestmark = pytest.mark.gpu
gpu = T.gpu
restate = lambda c, probes, k, off=0: search(c, c["qs"], probes, k, off)
# kind of rows -> (its suite's case, how that suite opens it, its restatement, its 1500-row list)
FAMS = {"f32": (lambda: T.make_case(33), T.open_case, restate, 5),
        "sq8": (lambda: N.case("sq8", 33), lambda api, c, **kw: N.open_case(api, c, "sq8", **kw), restate, 5),
        "u8": (lambda: BY.make_case("u8", 33), BY.open_case, restate, BY.LONG),
        "bits": (lambda: BI.make_case(100), BI.open_case, BI.restated, BI.LONG)}
MASKS = ("all", "none", "odd", "mod64", "long255", "long256", "long257", "long_last", "short")


def mask_of(c, long, what):
    """bool [n]: the rows a mask allows.  long*: only the first 255 / 256 / 257 rows of the long list (the filled tile's
    edge) or only its last row (chunk after chunk of carry, then a tile of one row); short: a bitmap that ends at n / 2."""
    n, rows = len(c["base"]), c["rows"][c["offsets"][long]:c["offsets"][long + 1]]
    m = np.zeros(n, dtype=bool)
    if what in ("all", "none"):
        m[:] = what == "all"
    elif what == "odd":
        m[1::2] = True
    elif what == "mod64":
        m[::64] = True
    elif what == "short":
        m[:n // 2] = True
    else:
        m[rows[-1:] if what == "long_last" else rows[:int(what[4:])]] = True
    return m


def cut_lists(c, mask):
    """The case with every list cut to the rows the mask allows, in list order."""
    keep = mask[c["rows"]]
    kept = np.concatenate([[0], np.cumsum(keep)])
    return dict(c, rows=c["rows"][keep], offsets=kept[c["offsets"]])


def make_filter(api, flat, mask, what, id_offset=0):
    if what == "short":                                                            # n_bits = n / 2: the ids beyond are not eligible
        return api.FlatIdFilter.from_mask(flat, np.concatenate([np.zeros(id_offset, dtype=bool), mask[:len(mask) // 2]]))
    return api.FlatIdFilter.from_ids(flat, np.flatnonzero(mask) + id_offset, n_bits=len(mask) + id_offset)


_tables = {}


def ip_table(c):
    """float32 [nq][n]: every query's exact score against every row, made once per base (the cases are left unchanged)."""
    if id(c["base"]) not in _tables:
        _tables[id(c["base"])] = XI.all_scores(c["base"], c["qs"]) if c["base"].dtype.kind == "f" else BX.table(c["base"], c["qs"], "ip")
    return _tables[id(c["base"])]


def ip_want(c, probes, k, off=0, mask=None, tab=None):
    """(ids, scores): per query the restated search over the rows of its probed lists, intersected with the mask."""
    tab, out = ip_table(c) if tab is None else tab, []
    for i, row in enumerate(probes):
        allowed = np.zeros(tab.shape[1], dtype=bool)
        for l in row[row >= 0]:
            allowed[c["rows"][c["offsets"][l]:c["offsets"][l + 1]]] = True
        out.append(BX.search(tab[i:i + 1], k, "ip", off, allowed if mask is None else allowed & mask))
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def ip_family(fmt, D):
    """(case, how to open it) of a format at a width, from the suite that owns the format."""
    if fmt == "f32":
        return T.make_case(D), T.open_case
    if fmt in ("u8", "i8"):
        return BY.make_case(fmt, D), BY.open_case
    return N.case(fmt, D), lambda api, c, **kw: N.open_case(api, c, fmt, **kw)


# an odd D, and one below, at and above the scan's slice: 32 dimensions, the narrow suite's SLICE, the 64-byte K step
IP_WIDTHS = [(f, D) for f, S in [("f32", 32)] + list(N.SLICE.items()) + [("u8", 64), ("i8", 64)] for D in (3, S - 1, S, S + 1)]


@pytest.mark.parametrize("fmt,D", IP_WIDTHS)
def test_inner_product_at_the_width_edges(gpu, fmt, D):
    """The suite's own lists and probes at top_k 100, host and device forms, a non-zero id_offset above the slice; base
    values and queries of both signs (fp32, narrow, i8), so negative scores reach the sink and the merge; and a probe of
    two short lists, fewer than top_k rows, where -inf padding must sort behind negative scores."""
    import torch
    c, open_case = ip_family(fmt, D)
    off = 1000 if D % 32 == 1 else 0
    few = np.tile(np.array([[1, 7 if fmt not in ("u8", "i8") else 12]], dtype=np.int32), (len(c["qs"]), 1))
    flat, ivf = open_case(gpu, c, id_offset=off)
    with flat, ivf:
        want = ip_want(c, c["probes"], 100, off)
        assert same(ivf.search_probes_ip(c["qs"], c["probes"], 100), want)
        got = ivf.search_probes_ip_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(c["probes"]).cuda(), 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
        want = ip_want(c, few, 100, off)
        assert fmt == "u8" or (want[1][want[0] >= 0] < 0).any()                     # negative scores in front of the padding
        assert (want[0] < 0).any() and same(ivf.search_probes_ip(c["qs"], few, 100), want)


def test_unsigned_bytes_at_the_extremes(gpu):
    """Rows and queries all 0, all 255 and mixed at D = 2048, where the integer score reaches 2048 * 255^2, near 2^31."""
    rng = np.random.default_rng(3)
    n, D = 600, 2048
    base = rng.integers(0, 256, (n, D), dtype=np.uint8)
    base[0::3], base[1::3] = 0, 255
    qs = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8)] + list(rng.integers(0, 256, (4, D), dtype=np.uint8)))
    c = dict(base=base, qs=qs, labels=(np.arange(n) % 4 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 3)
    probes = np.tile(np.arange(3, dtype=np.int32), (len(qs), 1))
    with gpu.FlatIndexU8(base) as flat, gpu.FlatIVFBytes.from_labels(flat, c["labels"], 3) as ivf:
        want = ip_want(c, probes, 100)
        assert want[1].max() == F32(2048 * 255 * 255) and same(ivf.search_probes_ip(qs, probes, 100), want)


@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_two_slices_of_queries_by_inner_product(gpu, kind):
    """2049 queries: the second slice takes its queries, and an unsigned handle its query terms, from past the first; a
    signed handle has no term arrays in either."""
    import torch
    dtype, lower = BY.KINDS[kind]
    rng = np.random.default_rng(4)
    as_kind = lambda a: (a - lower).astype(dtype)
    c = dict(base=as_kind(rng.integers(0, 256, (300, 4))), qs=as_kind(rng.integers(0, 256, (2049, 4))),
             labels=(np.arange(300) % 4 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 3)
    probes = (np.arange(2049) % 3).astype(np.int32)[:, None]
    with (gpu.FlatIndexU8 if kind == "u8" else gpu.FlatIndexI8)(c["base"]) as flat, gpu.FlatIVFBytes.from_labels(flat, c["labels"], 3) as ivf:
        want = ip_want(c, probes, 10)
        assert same(ivf.search_probes_ip(c["qs"], probes, 10), want)
        got = ivf.search_probes_ip_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(probes).cuda(), 10)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_the_coarse_step_by_inner_product(gpu, fmt):
    """probe_ip is the exact search_ip over the centroids (byte queries widened), the tie going to the lower list;
    search_ip is probe_ip + search_probes_ip, host and device forms."""
    import torch
    c, open_case = ip_family(fmt, 33)
    flat, ivf = open_case(gpu, c)
    with flat, ivf:
        lists, scores = ivf.probe_ip(c["qs"], 5)
        assert same((lists, scores), XI.search(c["cents"], c["qs"].astype(F32), 5))
        assert all(list(row).index(0) + 1 == list(row).index(1) for row in lists if 0 in row[:-1])  # the tie
        want = ip_want(c, lists, 100)
        assert same(ivf.search_ip(c["qs"], 5, 100), want) and same(ivf.search_probes_ip(c["qs"], lists, 100), want)
        got = ivf.search_ip_torch(torch.from_numpy(c["qs"]).cuda(), 5, 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_filter_and_inner_product_and_what_exists(gpu, fmt):
    """Inner product under a filter; and search_probes_ip is the handle's own search_filtered_ip under a filter of the probed
    lists' rows (intersected with the id filter), at a non-zero id_offset."""
    c, open_case = ip_family(fmt, 33)
    long = FAMS[fmt][3]
    mask = mask_of(c, long, "odd")
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf, make_filter(gpu, flat, mask, "odd", 7) as filt:
        assert same(ivf.search_probes_ip(c["qs"], c["probes"], 100, id_filter=filt), ip_want(c, c["probes"], 100, 7, mask))
        probes = np.array([[long, 2, 7]], dtype=np.int32)
        union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
        with gpu.FlatIdFilter.from_ids(flat, union + 7) as lists, gpu.FlatIdFilter.from_ids(flat, union[mask[union]] + 7) as both:
            assert same(ivf.search_probes_ip(c["qs"][:1], probes, 100), flat.search_filtered_ip(c["qs"][:1], 100, lists))
            assert same(ivf.search_probes_ip(c["qs"][:1], probes, 100, id_filter=filt), flat.search_filtered_ip(c["qs"][:1], 100, both))


def test_argument_errors_come_before_any_device_call(gpu, lib):
    """NULL arguments and the limits, on a real structure, with a real and with no filter."""
    c = T.make_case(3)
    ids, dists = np.zeros((2, 8), dtype=np.int32), np.zeros((2, 8), dtype=F32)
    q, p = c["qs"][:2].copy(), np.zeros((2, 1), dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    flat, ivf = T.open_case(gpu, c)
    with flat, ivf, gpu.FlatIdFilter.from_mask(flat, np.ones(len(c["base"]), dtype=bool)) as filt:
        for name in ("dpq_flat_ivf_search_filtered", "dpq_flat_ivf_search_ip"):
            whole, given = getattr(lib, name), getattr(lib, name.replace("search", "search_probes"))
            assert whole(None, ptr(q), 2, 1, 1, ptr(ids), ptr(dists), None) == ERR_ARG
            assert whole(ivf._h, None, 2, 1, 1, ptr(ids), ptr(dists), filt._h) == ERR_ARG
            assert given(ivf._h, ptr(q), 2, None, 1, 1, ptr(ids), ptr(dists), filt._h) == ERR_ARG
            for nq, nprobe, top_k in ((-1, 1, 1), (2, 0, 1), (2, 1025, 1), (2, 1, 0), (2, 1, 2049)):
                assert whole(ivf._h, ptr(q), nq, nprobe, top_k, ptr(ids), ptr(dists), filt._h) == ERR_ARG
                assert given(ivf._h, ptr(q), nq, ptr(p), nprobe, top_k, ptr(ids), ptr(dists), None) == ERR_ARG
        assert lib.dpq_flat_ivf_probe_ip(ivf._h, ptr(q), 2, 0, ptr(ids), None) == ERR_ARG


@pytest.mark.parametrize("what", MASKS)
@pytest.mark.parametrize("fam", list(FAMS))
def test_filter_masks(gpu, fam, what):
    """The suite's own lists (0, 1, 255, 256, 257, 1500 ... rows, -1 and repeated probes, 0 to 17 queries per list) at
    top_k 100, host form; then the long list beside a short one at top_k 300, device form, where under "all" the sink is
    cut between filled tiles."""
    import torch
    make, open_case, restated, long = FAMS[fam]
    c = make()
    mask = mask_of(c, long, what)
    want_c = cut_lists(c, mask)
    flat, ivf = open_case(gpu, c)
    with flat, ivf, make_filter(gpu, flat, mask, what) as filt:
        assert filt.n_allowed == mask.sum()
        assert same(ivf.search_probes(c["qs"], c["probes"], 100, id_filter=filt), restated(want_c, c["probes"], 100))
        probes = np.tile(np.array([[long, 2]], dtype=np.int32), (len(c["qs"]), 1))
        got = ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(probes).cuda(), 300, id_filter=filt)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), restated(want_c, probes, 300))


@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("fam", ["f32", "u8"])
def test_the_answers_do_not_depend_on_the_group(gpu, monkeypatch, fam, G):
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    make, open_case, restated, long = FAMS[fam]
    c = make()
    mask = mask_of(c, long, "odd")
    flat, ivf = open_case(gpu, c)
    with flat, ivf, make_filter(gpu, flat, mask, "odd") as filt:
        assert same(ivf.search_probes(c["qs"], c["probes"], 100, id_filter=filt), restated(cut_lists(c, mask), c["probes"], 100))
        assert same(ivf.search_probes_ip(c["qs"], c["probes"], 100), ip_want(c, c["probes"], 100))


@pytest.mark.parametrize("fam", list(FAMS))
def test_it_agrees_with_what_exists(gpu, fam):
    """No filter and the all-ones filter are today's search_probes; a filtered answer is the handle's own search_filtered
    under the intersection of the filter with the probed lists; the coarse step does not see the filter.  All at a
    non-zero id_offset, which a filter's ids carry."""
    make, open_case, restated, long = FAMS[fam]
    c = make()
    flat, ivf = open_case(gpu, c, id_offset=7)
    with flat, ivf:
        plain = ivf.search_probes(c["qs"], c["probes"], 100)
        assert same(plain, restated(c, c["probes"], 100, 7)) and same(plain, ivf.search_probes(c["qs"], c["probes"], 100, id_filter=None))
        with make_filter(gpu, flat, mask_of(c, long, "all"), "all", 7) as ones:
            assert same(plain, ivf.search_probes(c["qs"], c["probes"], 100, id_filter=ones))
        for what in ("odd", "short"):
            mask = mask_of(c, long, what)
            probes = np.array([[long, 2, 7]], dtype=np.int32)
            union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
            with make_filter(gpu, flat, mask, what, 7) as filt, gpu.FlatIdFilter.from_ids(flat, union[mask[union]] + 7) as both:
                assert same(ivf.search_probes(c["qs"][:1], probes, 100, id_filter=filt), flat.search_filtered(c["qs"][:1], 100, both))
                lists, _ = ivf.probe(c["qs"], 5)
                want = restated(cut_lists(c, mask), lists, 100, 7)
                assert same(ivf.search(c["qs"], 5, 100, id_filter=filt), want)
                assert same(ivf.search_probes(c["qs"], lists, 100, id_filter=filt), want)


def test_what_is_refused(gpu):
    c = T.make_case(33)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    flat, ivf = T.open_case(gpu, c)
    with flat, ivf, gpu.FlatIndex(c["base"]) as other, gpu.FlatIdFilter.from_mask(other, np.ones(len(c["base"]), dtype=bool)) as alien:
        import torch
        assert status(lambda: ivf.search_probes(c["qs"], c["probes"], 10, id_filter=alien)) == ERR_ARG
        assert status(lambda: ivf.search(c["qs"], 2, 10, id_filter=alien)) == ERR_ARG
        assert status(lambda: ivf.search_torch(torch.from_numpy(c["qs"]).cuda(), 2, 10, id_filter=alien)) == ERR_ARG
        with pytest.raises(TypeError):
            ivf.search_probes(c["qs"], c["probes"], 10, id_filter=np.ones(4, dtype=np.uint32))
        with gpu.FlatIdFilter.from_mask(flat, np.ones(len(c["base"]), dtype=bool)) as own:      # the next call works
            assert same(ivf.search_probes(c["qs"], c["probes"], 10, id_filter=own), search(c, c["qs"], c["probes"], 10))
    b = BI.make_case(100)
    flat, ivf = BI.open_case(gpu, b)
    with flat, ivf:                                                                # binary rows have no inner product
        assert status(lambda: ivf.search_probes_ip(b["qs"], b["probes"], 10)) == ERR_ARG
        assert status(lambda: ivf.search_ip(b["qs"], 2, 10)) == ERR_ARG and status(lambda: ivf.probe_ip(b["qs"], 2)) == ERR_ARG
        assert same(ivf.search_probes(b["qs"], b["probes"], 10), BI.restated(b, b["probes"], 10))
