"""IVF search over half-precision and scalar-quantised vectors (include/deltapq_amd.h "IVF search over raw vectors",
DESIGN.md 5.23).  The reference is tests/_flat_ivf_restatement.py over the fp32 rows the handle stands for -- the stored
16-bit patterns widened (tests/_half_restatement.py), the stored codes decoded (tests/_sq_restatement.py) -- and the handle is
opened from those very patterns and codes.  The GPU meets it bit for bit: ids, fp32 bits, -1 / +inf."""
import ctypes

import numpy as np
import pytest

import _half_restatement as H
import _sq_restatement as S
import test_ivf_flat as T
from _flat_ivf_restatement import lists_from_labels, same, search, search_at

F32 = np.float32
ERR_ARG, ERR_STATE = -1, -7
FMTS = ("f16", "bf16", "sq8", "sq4")
SLICE = {"f16": 32, "bf16": 32, "sq8": 64, "sq4": 128}      # dimensions of the scan's slice of 16 stored words
WIDTHS = [(f, D) for f in FMTS for D in (3, SLICE[f] - 1, SLICE[f], SLICE[f] + 1, 9 * SLICE[f] // 4)]
gpu = T.gpu
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def store(fmt, rows=None, stored=None, quant=None):
    """(what the handle is opened from, the fp32 rows it stands for): of fp32 rows narrowed or encoded under the quantiser
    trained on them, or of given patterns / packed codes."""
    if fmt in H.FORMATS:
        stored = H.narrow(rows, fmt) if stored is None else stored
        return (stored,), H.widen(stored, fmt)
    bits = 8 if fmt == "sq8" else 4
    lo, step = S.train(rows, bits) if quant is None else quant
    stored = S.encode(rows, lo, step, bits) if stored is None else stored
    return (stored, lo, step, bits), S.decode(stored, lo, step, bits)


def open_flat(api, fmt, args, id_offset=0):
    if fmt in H.FORMATS:
        return api.FlatIndexHalf(args[0], fmt, id_offset=id_offset)
    return api.FlatIndexSQ(*args, id_offset=id_offset)


def case(fmt, D):
    """test_ivf_flat's case at D with the base replaced by the rows the narrow handle stands for; built once."""
    def make():
        c = dict(T.make_case(D))
        c["args"], c["base"] = store(fmt, c["base"])
        return c
    return memo((fmt, D), make)


def open_case(api, c, fmt, id_offset=0, centroids=True):
    flat = open_flat(api, fmt, c["args"], id_offset)
    return flat, api.FlatIVF.from_labels(flat, c["labels"], T.NLIST, centroids=c["cents"] if centroids else None)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,D", WIDTHS)
def test_probed_lists_at_the_width_edges(gpu, fmt, D):
    """An odd D (the spare nibble, every format's padding), one below, at and above the slice, two slices and a fraction;
    test_ivf_flat's lists (0, 1, 255, 256, 257 rows, the long list, a row in no list, duplicated rows), its queries per
    list and its -1 and repeated probes; a non-zero id_offset above the slice; host and device forms."""
    import torch
    c = case(fmt, D)
    off = 1000 if D == SLICE[fmt] + 1 else 0
    flat, ivf = open_case(gpu, c, fmt, id_offset=off)
    with flat, ivf:
        want = search(c, c["qs"], c["probes"], 100, id_offset=off)
        assert same(ivf.search_probes(c["qs"], c["probes"], 100), want)
        got = ivf.search_probes_torch(torch.from_numpy(c["qs"]).cuda(), torch.from_numpy(c["probes"]).cuda(), 100)
        assert same((got[0].cpu().numpy(), got[1].cpu().numpy()), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_extreme_stored_values(gpu, fmt):
    """fp16: +-0, the smallest and the largest subnormal, the largest finite value.  bf16: +-0 and +-2^60, whose
    squares summed over D stay finite.  Codes: 0 and the top code, a dimension with step 0, negative lo."""
    rng = np.random.default_rng(7)
    n, D = 600, 40
    if fmt in H.FORMATS:
        edge = {"f16": [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF, 0x3C00, 0xB555],
                "bf16": [0x0000, 0x8000, 0x5D80, 0xDD80, 0x3F80, 0xBEAB, 0x0080]}[fmt]
        args, w = store(fmt, stored=rng.choice(np.array(edge, dtype=np.uint16), size=(n, D)))
    else:
        bits = 8 if fmt == "sq8" else 4
        top = S.levels(bits)
        lo, step = (-3 * rng.random(D)).astype(F32), rng.random(D).astype(F32)
        step[5], lo[6] = 0, 2.5
        codes = rng.choice(np.array([0, top, 1, top // 2], dtype=np.uint8), size=(n, D))
        args, w = store(fmt, stored=S.pack(codes, bits), quant=(lo, step))
    c = dict(base=w, labels=(np.arange(n) % 4 - 1).astype(np.int32))
    c["offsets"], c["rows"] = lists_from_labels(c["labels"], 3)
    qs, probes = rng.standard_normal((20, D)).astype(F32), np.tile(np.arange(3, dtype=np.int32), (20, 1))
    with open_flat(gpu, fmt, args) as flat, gpu.FlatIVF.from_labels(flat, c["labels"], 3) as ivf:
        assert same(ivf.search_probes(qs, probes, 100), search(c, qs, probes, 100))


@pytest.mark.gpu
@pytest.mark.parametrize("top_k,G", [(1, 16), (257, 16), (2048, 16), (100, 1), (100, 2), (100, 4), (100, 8), (100, 16)])
@pytest.mark.parametrize("fmt", FMTS)
def test_the_sink_and_the_group(gpu, monkeypatch, fmt, top_k, G):
    """Asked for G = 16 with nprobe 9: top_k 1; 257, where the buffers double; 2048, where G is the 4 that fit beside the
    tile and the merge takes two rounds.  Then every G at top_k 100: the answer does not depend on it."""
    monkeypatch.setenv("DPQ_DEV", "1")
    monkeypatch.setenv("DPQ_FLAT_IVF_GROUP", str(G))
    c = case(fmt, 33)
    q = np.arange(T.NQ)
    probes = c["probes"] if top_k == 100 else np.stack([(3 + q + j) % T.NLIST for j in range(9)], 1).astype(np.int32)
    ks = (100,) if top_k == 100 else (1, 257, 2048)
    want = memo((fmt, ks), lambda: search_at(c, c["qs"], probes, ks))[top_k]
    flat, ivf = open_case(gpu, c, fmt)
    with flat, ivf:
        assert same(ivf.search_probes(c["qs"], probes, top_k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_it_agrees_with_what_exists(gpu, fmt):
    """The fp32 FlatIVF over the widened or decoded rows (search, probe with two equal centroids, search = probe +
    search_probes), the narrow handle's own filtered exact search, and ivf_assign's lists."""
    c = case(fmt, 33)
    flat, ivf = open_case(gpu, c, fmt, id_offset=7)
    wide = gpu.FlatIndex(c["base"], id_offset=7)
    with flat, ivf, wide, gpu.FlatIVF.from_labels(wide, c["labels"], T.NLIST, centroids=c["cents"]) as ref:
        lists, dists = ivf.probe(c["qs"], 5)
        assert same((lists, dists), ref.probe(c["qs"], 5))
        assert all(list(row).index(0) + 1 == list(row).index(1) for row in lists if 0 in row[:-1])  # the tie
        got = ivf.search(c["qs"], 5, 100)
        assert same(got, ref.search(c["qs"], 5, 100)) and same(got, ivf.search_probes(c["qs"], lists, 100))
        probes = np.array([[5, 2, 7]], dtype=np.int32)
        union = np.concatenate([c["rows"][c["offsets"][l]:c["offsets"][l + 1]] for l in probes[0]])
        with gpu.FlatIdFilter.from_ids(flat, union + 7) as filt:
            assert same(ivf.search_probes(c["qs"][:1], probes, 100), flat.search_filtered(c["qs"][:1], 100, filt))
        with gpu.FlatIVF.build(flat, c["cents"]) as built:
            labels, _ = gpu.ivf_assign(c["cents"], c["base"])
            want, got = lists_from_labels(labels, T.NLIST), built.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1] + 7)


@pytest.mark.gpu
def test_what_stays_refused(gpu):
    c = case("f16", 33)
    status = lambda fn: pytest.raises(gpu.DpqError, fn).value.status
    labels8 = np.zeros(8, dtype=np.int32)
    with gpu.FlatIndexU8(np.zeros((8, 4), dtype=np.uint8)) as b, gpu.FlatIndexBits(np.zeros((8, 1), dtype=np.uint8), 8) as bits:
        assert status(lambda: gpu.FlatIVF.from_labels(b, labels8, 2)) == ERR_ARG
        assert status(lambda: gpu.FlatIVF.from_labels(bits, labels8, 2)) == ERR_ARG
    flat, ivf = open_case(gpu, c, "f16", centroids=False)
    with flat, ivf:
        assert status(lambda: gpu.FlatIVFBytes.from_labels(flat, c["labels"], T.NLIST)) == ERR_ARG
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        qb, ids, dists = np.zeros((T.NQ, 33), dtype=np.uint8), np.zeros((T.NQ, 10), dtype=np.int32), np.zeros((T.NQ, 10), dtype=F32)
        assert ivf._lib.dpq_flat_ivf_search_probes_bytes(ivf._h, ptr(qb), T.NQ, ptr(c["probes"]), 4, 10, ptr(ids), ptr(dists)) == ERR_ARG
        assert status(lambda: ivf.search(c["qs"], 2, 10)) == ERR_STATE
        assert same(ivf.search_probes(c["qs"], c["probes"], 10), search(c, c["qs"], c["probes"], 10))  # the next call works
