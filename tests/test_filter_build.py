"""Filter construction on the GPU (dpq_filter_create_device / _ids / _range / _vec, dpq_filter_combine,
dpq_filter_to_bitmap, dpq_bitmap_from_*_device).

Two independent yardsticks.  (1) The host path as it was before these constructors existed: dpq_filter_create from the
equivalent host bitmap, and dpq_bitmap_to_dfs in front of it for bitmaps over vector ids.  (2) A restatement in plain
numpy (tests/_filter_build_restatement.py).  A filter from a device constructor must read back (dpq_filter_to_bitmap
over [0, id_hi + 70)) and count (dpq_filter_count) exactly as both; searches through it must return the same ids and
the same distance bits as through the host-built filter.

Handles come from one fixed table (HANDLES); its coverage is asserted by test_handle_table_covers_the_corners."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import _filter_build_restatement as R
import _option_matrix as om
from conftest import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("dpq_filter_create_device", "dpq_filter_create_ids", "dpq_filter_create_ids_device",
               "dpq_filter_create_range", "dpq_set_vec_ids", "dpq_filter_create_vec", "dpq_filter_create_vec_device",
               "dpq_filter_combine", "dpq_filter_to_bitmap", "dpq_bitmap_from_mask_device", "dpq_bitmap_from_ids_device")


# ---- the handle table ---------------------------------------------------------------------------------------------

def _case(n, **kw):
    kw.setdefault("seed", 1000 + n)
    return om.make_case(n, **kw)


def _handles():
    """[(label, case, rank, plain)]: sizes {1, 2, 3, 63, 64, 65, 129, 4097} over every placement."""
    out = [("whole_n%d" % n, _case(n), 0, False) for n in (1, 2, 3, 63, 64, 65, 129, 4097)]
    out += [("shard%d_of3_n4097_cps1" % r, _case(4097, cps=1, shards=3), r, False) for r in range(3)]
    out += [("prefix_even_86_of_129", _case(129, num_codes=86), 0, False),
            ("prefix_odd_85_of_129", _case(129, num_codes=85), 0, False),
            ("prefix_odd_2731_of_4097", _case(4097, num_codes=2731), 0, False)]
    # an even prefix in two shards: rank 0 is a shard of an even-N index that does not hold its last node
    out += [("prefix_even_2730_of_4097_shard%d_of2" % r, _case(4097, cps=1, shards=2, num_codes=2730), r, False)
            for r in range(2)]
    for off in (1_000_000, 1_000_003):
        for n in (64, 65):                                                        # the global tail: N = off + n
            out.append(("part_off%d_n%d_tail_N%s" % (off, n, "even" if (off + n) % 2 == 0 else "odd"),
                        _case(n, offset=off, global_n=off + n), 0, False))
        out.append(("part_off%d_n129_not_tail" % off, _case(129, offset=off, global_n=off + 129 + om.SLACK), 0, False))
    out.append(("part_off1000003_n4097_tail_Neven", _case(4097, offset=1_000_003, global_n=1_000_003 + 4097), 0, False))
    out += [("plain_n64", _case(64), 0, True), ("plain_n4097_cps1", _case(4097, cps=1), 0, True)]
    out.append(("m16_n64", _case(64, mkd=(16, 256, 8)), 0, False))
    out.append(("m16_n4097", _case(4097, mkd=(16, 256, 8)), 0, False))
    return out


HANDLES = _handles()
HANDLE_IDS = [h[0] for h in HANDLES]


@functools.lru_cache(maxsize=None)
def _inputs(label):
    case = next(h[1] for h in HANDLES if h[0] == label)
    return om.build_inputs(case)


class Geom:
    """What the restatement needs of a handle, and the id span every read-back covers."""

    def __init__(self, base, n_local, N, plain):
        self.base, self.n_local, self.N, self.plain = int(base), int(n_local), int(N), bool(plain)
        rep = R.reported(base, n_local, N, plain)
        self.id_hi = int(rep.max()) + 1 if n_local else self.base
        self.span = self.id_hi + 70
        self.even_tail = (not plain) and N % 2 == 0 and self.base <= N - 1 < self.base + self.n_local

    def args(self):
        return self.base, self.n_local, self.N, self.plain


def expected_geom(label, case, rank, plain):
    """The handle's geometry from the host transcoder alone (no GPU)."""
    if plain:
        return Geom(0, case["n"], case["n"], True)
    lo, hi = om.handle_bounds(case, _inputs(label))[rank]
    return Geom(lo, hi - lo, om.n_total(case), False)


def test_handle_table_covers_the_corners():
    geoms = {h[0]: expected_geom(*h) for h in HANDLES}
    assert {h[1]["n"] for h in HANDLES} == {1, 2, 3, 63, 64, 65, 129, 4097}
    assert any(g.base & 31 for g in geoms.values()), "no handle with id_base & 31 != 0"
    assert any(g.even_tail for g in geoms.values()), "no handle holds an even-N last node"
    assert any(h[1]["shards"] > 1 and not h[3] and geoms[h[0]].N % 2 == 0 and not geoms[h[0]].even_tail for h in HANDLES), \
        "no shard of an even-N index that does not hold its last node"
    assert any(g.n_local % (64 * h[1]["cps"]) for h, g in zip(HANDLES, geoms.values())), \
        "no handle with n_local off its segment size"
    assert any(h[3] for h in HANDLES) and any(h[1]["M"] == 16 for h in HANDLES)
    assert sum(h[1]["shards"] == 3 and h[1]["cps"] == 1 and h[1]["n"] == 4097 for h in HANDLES) == 3
    for off in (1_000_000, 1_000_003):
        parts = [g for h, g in zip(HANDLES, geoms.values()) if h[1]["offset"] == off]
        kinds = {(g.base + g.n_local == g.N, g.N % 2) for g in parts}                # (the global tail?, parity of N)
        assert (True, 0) in kinds and (True, 1) in kinds and any(not tail for tail, _ in kinds), kinds
    prefixes = [h[1]["num_codes"] % 2 for h in HANDLES if h[1]["num_codes"]]
    assert 0 in prefixes and 1 in prefixes


# ---- CPU: binding and argument checks -------------------------------------------------------------------------------

def test_new_symbols_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    names = {name for name, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in names, name
        assert name + "(" in header, name
        assert hasattr(raw, name), name


def test_constructor_argument_checks(lib):
    buf = np.ones(8, dtype=np.uint32)
    p = ctypes.c_void_p(buf.ctypes.data)
    fake = ctypes.c_void_p(0x1000)          # never dereferenced: the argument checks come first
    calls = [
        lambda x, o: lib.dpq_filter_create_device(x, p, 100, None, o),
        lambda x, o: lib.dpq_filter_create_ids(x, p, 4, 0, o),
        lambda x, o: lib.dpq_filter_create_ids_device(x, p, 4, 1, None, o),
        lambda x, o: lib.dpq_filter_create_range(x, 0, 10, o),
        lambda x, o: lib.dpq_filter_create_vec(x, p, 100, o),
        lambda x, o: lib.dpq_filter_create_vec_device(x, p, 100, None, o),
        lambda x, o: lib.dpq_filter_combine(x, 0, fake, fake, o),
    ]
    for call in calls:
        out = ctypes.c_void_p(1)
        assert call(None, ctypes.byref(out)) == -1           # NULL index
        assert out.value is None                             # *out is cleared
        assert call(fake, None) == -1                        # NULL out
    bad = [
        lambda o: lib.dpq_filter_create_device(fake, p, -1, None, o),        # n_bits < 0
        lambda o: lib.dpq_filter_create_device(fake, None, 5, None, o),      # NULL with a size
        lambda o: lib.dpq_filter_create_vec(fake, p, -1, o),
        lambda o: lib.dpq_filter_create_vec(fake, None, 5, o),
        lambda o: lib.dpq_filter_create_vec_device(fake, p, -1, None, o),
        lambda o: lib.dpq_filter_create_vec_device(fake, None, 5, None, o),
        lambda o: lib.dpq_filter_create_ids(fake, p, -1, 0, o),              # n < 0
        lambda o: lib.dpq_filter_create_ids(fake, None, 3, 0, o),
        lambda o: lib.dpq_filter_create_ids_device(fake, p, -1, 0, None, o),
        lambda o: lib.dpq_filter_create_ids_device(fake, None, 3, 0, None, o),
        lambda o: lib.dpq_filter_create_range(fake, 7, 6, o),                # lo > hi
        lambda o: lib.dpq_filter_combine(fake, 5, fake, fake, o),            # unknown op
        lambda o: lib.dpq_filter_combine(fake, -1, fake, fake, o),
        lambda o: lib.dpq_filter_combine(fake, 4, fake, fake, o),            # NOT with b
        lambda o: lib.dpq_filter_combine(fake, 0, fake, None, o),            # AND without b
        lambda o: lib.dpq_filter_combine(fake, 0, None, fake, o),
    ]
    for i, call in enumerate(bad):
        out = ctypes.c_void_p(1)
        assert call(ctypes.byref(out)) == -1, i
        assert out.value is None, i
    assert lib.dpq_filter_to_bitmap(None, p, 100) == -1
    assert lib.dpq_filter_to_bitmap(fake, p, -1) == -1
    assert lib.dpq_filter_to_bitmap(fake, None, 5) == -1
    assert lib.dpq_set_vec_ids(None, p, 8) == -1
    assert lib.dpq_set_vec_ids(fake, p, -1) == -1
    assert lib.dpq_set_vec_ids(fake, None, 8) == -1
    assert lib.dpq_bitmap_from_mask_device(p, -1, p, 0, None) == -1
    assert lib.dpq_bitmap_from_mask_device(None, 5, p, 0, None) == -1
    assert lib.dpq_bitmap_from_mask_device(p, 5, None, 0, None) == -1
    assert lib.dpq_bitmap_from_ids_device(p, -1, 10, p, 0, None) == -1
    assert lib.dpq_bitmap_from_ids_device(p, 4, -1, p, 0, None) == -1
    assert lib.dpq_bitmap_from_ids_device(None, 4, 10, p, 0, None) == -1
    assert lib.dpq_bitmap_from_ids_device(p, 4, 10, None, 0, None) == -1


def test_restatement_on_a_hand_case():
    # base 4, five nodes, N = 9 (odd): ids 4 .. 8; N = 8 on a part [4, 8): node 7 is reported as 8
    assert R.reported(4, 5, 9, False).tolist() == [4, 5, 6, 7, 8]
    assert R.reported(4, 4, 8, False).tolist() == [4, 5, 6, 8]
    assert R.reported(4, 4, 8, True).tolist() == [4, 5, 6, 7]
    m = np.zeros(8, dtype=bool)
    m[[5, 7]] = True
    assert R.local_bits(4, 4, 8, False, R.in_mask(m)).tolist() == [False, True, False, False]     # bit 7 governs nothing
    assert R.local_bits(4, 4, 8, True, R.in_mask(m)).tolist() == [False, True, False, True]
    assert R.as_reported_mask([1, 0, 0, 1], 4, 4, 8, False, 10).nonzero()[0].tolist() == [4, 8]
    assert R.local_bits_vec([3, 9, 5], R.in_mask(m)).tolist() == [False, False, True]


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@contextlib.contextmanager
def open_handle(api, label):
    _, case, rank, plain = next(h for h in HANDLES if h[0] == label)
    inp = _inputs(label)
    if plain:
        idx = api.DeltaPQIndex.open_plain(inp["codes"], K=case["K"], chunks_per_segment=case["cps"])
    else:
        idx = api.DeltaPQIndex.open_memory(inp["payload"], case["n"], case["M"], case["K"], **om.open_kwargs(case, rank))
    with idx:
        info = idx.info()
        g = Geom(info["node_lo"], info["node_hi"] - info["node_lo"], info["n_codes_total"], plain)
        e = expected_geom(label, case, rank, plain)
        assert g.args() == e.args(), "%s: the handle is not what the table expects" % label
        yield idx, g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_filter(api, idx, g, f, host_mask, want_bits, what):
    """f against the host-built filter of host_mask (bool over reported ids) and the restatement's local bits."""
    want = R.as_reported_mask(want_bits, *g.args(), g.span)
    with api.IdFilter.from_mask(idx, host_mask) as fh:
        host, host_n = fh.to_mask(g.span), fh.n_allowed
    got, got_n = f.to_mask(g.span), f.n_allowed
    f.close()
    assert np.array_equal(host, want), "%s: the host path and the restatement disagree" % what
    assert np.array_equal(got, want), "%s: bits differ at reported ids %s" % (what, np.flatnonzero(got != want)[:8])
    assert got_n == host_n == int(np.count_nonzero(want_bits)), "%s: n_allowed %d, host %d, restatement %d" % (
        what, got_n, host_n, int(np.count_nonzero(want_bits)))


def bitmap_sources(g, rng):
    """[(name, bool mask over reported ids)]"""
    lo = max(0, g.base - 40)
    def random(frac):
        m = np.zeros(g.span, dtype=bool)
        m[lo:] = rng.random(g.span - lo) < frac
        return m
    cut = g.base + max(1, g.n_local // 2)
    if cut % 32 == 0:
        cut += 1
    out = [("density 0.5", random(0.5)), ("density 0.02", random(0.02)), ("ones", np.ones(g.span, dtype=bool)),
           ("zeros", np.zeros(g.span, dtype=bool)), ("n_bits 0", np.zeros(0, dtype=bool)),
           ("cut at %d" % cut, np.ones(cut, dtype=bool)), ("far beyond", np.ones(g.id_hi + 100_003, dtype=bool))]
    if not g.plain and g.N % 2 == 0 and g.N < g.span:
        a, b = random(0.5), random(0.5)
        a[g.N], a[g.N - 1] = True, False
        b[g.N], b[g.N - 1] = False, True
        out += [("bit N without N - 1", a), ("bit N - 1 without N", b)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("label", HANDLE_IDS)
def test_bitmaps_over_reported_ids(gpu, label):
    rng = np.random.default_rng(11)
    with open_handle(gpu, label) as (idx, g):
        for name, m in bitmap_sources(g, rng):
            want = R.local_bits(*g.args(), R.in_mask(m))
            check_filter(gpu, idx, g, gpu.IdFilter.from_mask_torch(idx, dev(m)), m, want, "%s bitmap %s" % (label, name))


def id_lists(g, rng):
    lo, hi = max(0, g.base - 60), g.id_hi + 60
    rand = rng.integers(lo, hi, size=3 * g.n_local + 5)
    neg = np.concatenate([rand, np.full(17, -1), [-7, -2 ** 31]])
    rng.shuffle(neg)
    others = np.concatenate([np.arange(max(0, g.base - 200), g.base), np.arange(g.id_hi, g.id_hi + 200),
                             g.base + rng.integers(0, g.n_local, size=3)])
    pool = rng.choice(np.arange(max(0, g.base - 300), g.id_hi + 300), 200, replace=False)
    out = [("random with duplicates", rand), ("negatives", neg), ("ids of other shards", others), ("empty", np.zeros(0)),
           ("300000 from 200", pool[rng.integers(0, 200, size=300_000)])]
    if not g.plain and g.N % 2 == 0:
        out += [("N and N - 1", np.array([g.N, g.N - 1])), ("N", np.array([g.N])), ("N - 1", np.array([g.N - 1]))]
    return [(name, np.asarray(a, dtype=np.int32)) for name, a in out]


@pytest.mark.gpu
@pytest.mark.parametrize("label", HANDLE_IDS)
def test_id_lists(gpu, label):
    rng = np.random.default_rng(12)
    with open_handle(gpu, label) as (idx, g):
        for name, ids in id_lists(g, rng):
            listed = np.zeros(g.span, dtype=bool)
            listed[ids[(ids >= 0) & (ids < g.span)]] = True
            for invert in (False, True):
                m = ~listed if invert else listed
                want = R.local_bits(*g.args(), lambda r: np.isin(r, ids[ids >= 0]) != invert)
                what = "%s ids %s invert=%d" % (label, name, invert)
                check_filter(gpu, idx, g, gpu.IdFilter.from_ids_torch(idx, dev(ids), invert=invert), m, want, what + " (device)")
                check_filter(gpu, idx, g, gpu.IdFilter.from_ids(idx, ids, invert=invert), m, want, what + " (host ids)")


@pytest.mark.gpu
@pytest.mark.parametrize("label", HANDLE_IDS)
def test_ranges(gpu, label):
    with open_handle(gpu, label) as (idx, g):
        mid = g.base + g.n_local // 2
        ranges = [(g.base + 1, g.base + 1), (0, 0), (0, g.id_hi), (0, g.span + 1000), (max(0, g.base - 10), mid),
                  (mid, g.id_hi + 10), (g.base, g.base + 1), (g.id_hi - 1, g.id_hi), (g.id_hi + 5, g.id_hi + 9), (-5, mid)]
        if not g.plain and g.N % 2 == 0:
            ranges += [(g.N - 1, g.N + 1), (g.N, g.N + 1), (g.N - 1, g.N), (g.N - 2, g.N)]
        for lo, hi in ranges:
            m = np.zeros(g.span, dtype=bool)
            m[max(lo, 0):max(hi, 0)] = True
            want = R.local_bits(*g.args(), lambda r: (r >= lo) & (r < hi))
            check_filter(gpu, idx, g, gpu.IdFilter.from_range(idx, lo, hi), m, want, "%s range [%d, %d)" % (label, lo, hi))


@pytest.mark.gpu
@pytest.mark.parametrize("label", HANDLE_IDS)
def test_bitmaps_over_vector_ids(gpu, label):
    """vec_id: a random permutation shifted so that some entries lie at or beyond n_bits.  The host yardstick is
    dpq_bitmap_to_dfs over the whole index's map (the handle's slice filled in, 0xffffffff elsewhere) and
    dpq_filter_create of its output."""
    rng = np.random.default_rng(13)
    with open_handle(gpu, label) as (idx, g):
        with pytest.raises(gpu.DpqError) as e:
            gpu.IdFilter.from_vec_mask(idx, np.ones(4, dtype=bool))
        assert e.value.status == -7                       # DPQ_ERR_STATE before set_vec_ids
        for bad in (g.n_local + 1, g.n_local - 1):
            with pytest.raises(gpu.DpqError) as e:
                idx.set_vec_ids(np.zeros(bad, dtype=np.uint32))
            assert e.value.status == -1
        shift = max(1, g.n_local // 8)
        vec = (rng.permutation(g.n_local) + shift).astype(np.uint32)
        idx.set_vec_ids(vec)
        # the whole index's map; an odd length on a plain handle, which has no even-N rule
        L = g.N if not g.plain else g.N + 1 - g.N % 2
        whole = np.full(L, 0xffffffff, dtype=np.uint32)
        whole[g.base:g.base + g.n_local] = vec
        for name, vm in (("density 0.5", rng.random(g.n_local) < 0.5), ("ones", np.ones(g.n_local, dtype=bool)),
                         ("n_bits 0", np.zeros(0, dtype=bool)), ("covering", rng.random(g.n_local + shift + 40) < 0.5),
                         ("zeros", np.zeros(g.n_local, dtype=bool))):
            w, nb = gpu.IdFilter.pack_mask(vm)
            dfs_w, dfs_n = gpu.bitmap_to_dfs(w, nb, whole)
            m = gpu.IdFilter.unpack(dfs_w, dfs_n)
            want = R.local_bits_vec(vec, R.in_mask(vm))
            what = "%s vector-id bitmap %s" % (label, name)
            check_filter(gpu, idx, g, gpu.IdFilter.from_vec_mask(idx, vm), m, want, what + " (host words)")
            check_filter(gpu, idx, g, gpu.IdFilter.from_vec_mask_torch(idx, dev(vm)), m, want, what + " (device)")
            ids = np.concatenate([np.flatnonzero(vm), [-4, len(vm), len(vm) + 77]]).astype(np.int32)
            check_filter(gpu, idx, g, gpu.IdFilter.from_vec_ids_torch(idx, dev(ids), len(vm)), m, want, what + " (device ids)")
            check_filter(gpu, idx, g, gpu.IdFilter.from_vec_ids(idx, np.flatnonzero(vm), len(vm)), m, want, what + " (host ids)")


@pytest.mark.gpu
@pytest.mark.parametrize("label", HANDLE_IDS)
def test_combine(gpu, label):
    rng = np.random.default_rng(14)
    with open_handle(gpu, label) as (idx, g):
        ma = np.zeros(g.span, dtype=bool)
        ma[max(0, g.base - 40):] = rng.random(g.span - max(0, g.base - 40)) < 0.5
        ids = rng.integers(max(0, g.base - 60), g.id_hi + 60, size=g.n_local + 3).astype(np.int32)
        nodes = R.as_reported_mask(np.ones(g.n_local, dtype=bool), *g.args(), g.span)   # ids that name a node
        with gpu.IdFilter.from_mask_torch(idx, dev(ma)) as a, gpu.IdFilter.from_ids_torch(idx, dev(ids)) as b, \
                gpu.IdFilter.from_mask(idx, ma) as a_host:
            A, B = a.to_mask(g.span), b.to_mask(g.span)
            for name, f, want in (("and", a & b, A & B), ("or", a | b, A | B), ("andnot", a - b, A & ~B),
                                  ("xor", a ^ b, A ^ B), ("not", ~a, ~A & nodes), ("host and", a_host & b, A & B),
                                  ("not host", ~a_host, ~A & nodes)):
                with f:
                    assert np.array_equal(f.to_mask(g.span), want), "%s %s" % (label, name)
                    assert f.n_allowed == int(want.sum()), "%s %s: count" % (label, name)
            with ~a as na:
                assert na.n_allowed == g.n_local - a.n_allowed     # the padding bits stay 0
                with a & na as none, a | na as every, ~every as none2:
                    assert none.n_allowed == 0 and not none.to_mask(g.span).any()
                    assert every.n_allowed == g.n_local and none2.n_allowed == 0
            with gpu.IdFilter.from_range(idx, 0, 0) as z, ~z as full:
                assert z.n_allowed == 0 and full.n_allowed == g.n_local
                assert np.array_equal(full.to_mask(g.span), nodes)


@pytest.mark.gpu
def test_combine_refuses_filters_of_two_handles(gpu, lib):
    with open_handle(gpu, "whole_n129") as (i1, _), open_handle(gpu, "whole_n129") as (i2, _):
        with gpu.IdFilter.from_range(i1, 0, 50) as a, gpu.IdFilter.from_range(i2, 0, 50) as b:
            for x, p, q in ((i1, a, b), (i2, a, b), (i1, b, a), (i1, b, b)):
                out = ctypes.c_void_p(1)
                assert lib.dpq_filter_combine(x._h, 0, p._h, q._h, ctypes.byref(out)) == -1
                assert out.value is None
            out = ctypes.c_void_p(1)
            assert lib.dpq_filter_combine(i1._h, 4, b._h, None, ctypes.byref(out)) == -1
            with pytest.raises(gpu.DpqError) as e:
                a & b
            assert e.value.status == -1
            with pytest.raises(gpu.DpqError):               # and the searches' owner check holds for the new filters
                i2.query_batch_filtered(np.zeros((1, 128), dtype=np.float32), 1, a)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 4099])
def test_packing_helpers(gpu, lib, n):
    import torch
    rng = np.random.default_rng(n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_words = (n + 31) // 32
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None
    m = rng.random(n) < 0.4
    dm = dev(m)
    words = torch.full((n_words,), -1, dtype=torch.int32, device="cuda")     # (stale bits everywhere)
    assert lib.dpq_bitmap_from_mask_device(ptr(dm), n, ptr(words), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), gpu.IdFilter.pack_mask(m)[0])
    inside = rng.integers(0, max(n, 1), size=2 * n) if n else np.zeros(0, dtype=np.int64)
    ids = np.concatenate([inside, [-3, n, n + 5, 2 ** 31 - 1]]).astype(np.int32)
    rng.shuffle(ids)
    di = dev(ids)
    words = torch.full((n_words,), -1, dtype=torch.int32, device="cuda")
    assert lib.dpq_bitmap_from_ids_device(ptr(di), len(ids), n, ptr(words), 0, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(words.cpu().numpy().view(np.uint32), gpu.IdFilter.pack_ids(inside, n)[0])
    # an empty list clears the bitmap
    assert lib.dpq_bitmap_from_ids_device(None, 0, n, ptr(words), 0, stream) == 0
    torch.cuda.synchronize()
    assert not words.cpu().numpy().any()


# ---- GPU: searches ------------------------------------------------------------------------------------------------

NQ, TOP_K = 130, 100


@functools.lru_cache(maxsize=None)
def _search_case(n):
    from deltapq_amd import synth
    _, payload, _ = make_case(n, seed=900 + n % 97)
    return payload, synth.make_queries(NQ, 128, seed=901 + n % 97)


def assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": ids differ"
    assert np.array_equal(np.asarray(a[1]).view(np.uint32), np.asarray(b[1]).view(np.uint32)), what + ": distances differ"


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.5, 0.01])
@pytest.mark.parametrize("n", [20000, 100000])
def test_searches_through_device_built_filters(gpu, codebook, n, density):
    """20 000 codes: the level-0 path, no bootstrap; 100 000: the bootstrap.  Even N both: mask bit N governs the last node."""
    import torch
    payload, qs = _search_case(n)
    rng = np.random.default_rng(int(n + 1000 * density))
    g = Geom(0, n, n, False)
    rep = R.reported(*g.args())
    mask = rng.random(n + 1) < density
    allow, deny = rng.random(n + 1) < min(1.0, 2 * density), rng.random(n + 1) < 0.5
    vec = rng.permutation(n).astype(np.uint32)
    vmask = np.zeros(n, dtype=bool)
    vmask[vec] = mask[rep]
    r_lo, r_hi = n // 4, n // 4 + max(TOP_K // 2, int(density * n))
    rmask = np.zeros(n + 1, dtype=bool)
    rmask[r_lo:r_hi] = True
    ids = np.flatnonzero(mask).astype(np.int32)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        idx.set_vec_ids(vec)
        assert (idx.info()["bootstrap_bytes"] > 0) == (n >= 65536)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            want, want_n = idx.query_batch_filtered(qs, TOP_K, f), f.n_allowed
        builders = [
            ("from_mask_torch", lambda: gpu.IdFilter.from_mask_torch(idx, dev(mask))),
            ("from_ids_torch", lambda: gpu.IdFilter.from_ids_torch(idx, dev(ids))),
            ("from_ids (host list)", lambda: gpu.IdFilter.from_ids(idx, ids)),
            ("deny-list", lambda: gpu.IdFilter.from_ids_torch(idx, dev(np.flatnonzero(~mask).astype(np.int32)), invert=True)),
            ("from_vec_mask", lambda: gpu.IdFilter.from_vec_mask(idx, vmask)),
            ("from_vec_mask_torch", lambda: gpu.IdFilter.from_vec_mask_torch(idx, dev(vmask))),
            ("from_vec_ids_torch", lambda: gpu.IdFilter.from_vec_ids_torch(idx, dev(np.flatnonzero(vmask).astype(np.int32)), n)),
        ]
        for name, build in builders:
            with build() as f:
                assert f.n_allowed == want_n, name
                assert_same(idx.query_batch_filtered(qs, TOP_K, f), want, "n=%d density=%g %s" % (n, density, name))
        # a range, and a combination, against the host filters of their masks
        with gpu.IdFilter.from_mask(idx, rmask) as fh, gpu.IdFilter.from_range(idx, r_lo, r_hi) as f:
            assert_same(idx.query_batch_filtered(qs, TOP_K, f), idx.query_batch_filtered(qs, TOP_K, fh), "range")
        with gpu.IdFilter.from_mask(idx, allow & ~deny) as fh, gpu.IdFilter.from_mask_torch(idx, dev(allow)) as fa, \
                gpu.IdFilter.from_ids_torch(idx, dev(np.flatnonzero(deny).astype(np.int32))) as fd, ~fd as nfd, fa & nfd as f:
            assert f.n_allowed == fh.n_allowed
            assert_same(idx.query_batch_filtered(qs, TOP_K, f), idx.query_batch_filtered(qs, TOP_K, fh), "allow & ~deny")
        # device queries through a filter built from a device mask
        with gpu.IdFilter.from_mask_torch(idx, dev(mask)) as f:
            ti, td = idx.query_batch_filtered_torch(dev(qs), TOP_K, f)
            torch.cuda.synchronize()
            assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "query_batch_filtered_torch")


@pytest.mark.gpu
def test_two_shards_build_from_one_global_id_list(gpu, codebook):
    n, density = 100000, 0.01
    payload, qs = _search_case(n)
    rng = np.random.default_rng(5)
    mask = rng.random(n + 1) < density
    ids = np.flatnonzero(mask).astype(np.int32)
    rng.shuffle(ids)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(codebook)
        with gpu.IdFilter.from_mask(idx, mask) as f:
            want, want_n = idx.query_batch_filtered(qs, TOP_K, f), f.n_allowed
    parts, counts = [], 0
    for rank in range(2):
        with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, shard_rank=rank, shard_count=2) as idx:
            idx.set_codebook(codebook)
            with gpu.IdFilter.from_ids_torch(idx, dev(ids)) as f:
                counts += f.n_allowed
                parts.append(idx.query_batch_filtered(qs, TOP_K, f))
    assert counts == want_n
    merged = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert_same(merged, want, "two shards merged")
