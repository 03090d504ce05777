"""Filtered top-k, range search and code lookup crossed with every dpq_open_opts field, on ONE open handle per placement.

tests/_option_matrix.py holds the case table (fixed and seeded; each pytest id spells out every option), the references
(plain numpy over the oracle's per-code distances, by (distance bits, reported id)) and the call sequence.  Per handle of a
case -- the whole index, every shard, or the part -- the GPU test calls, in this order: query_batch (tie-aware against the
oracle), query_batch_filtered under three masks (all ones = the unfiltered bits; random; a few ids with bit N set and
bit N - 1 clear on the even-N tail; n_bits once beyond, once short of, once exactly the id range), range_search over the
six radius kinds, get_codes of the filtered rows with their padding, and query_batch again (the same bits).  Sharded
cases merge the per-shard rows and lists and compare them with the oracle's whole-index expectation.  Every query of
every case is checked; only answers are asserted, no counters, timings or plan internals.

Crossed: n (1 .. 70 001: one node, one segment at 64 chunks per segment, level 0 with filter levels, forced and automatic
bootstrap), (M, K, Ds), chunks_per_segment, batch_decode, bootstrap, flags, stream_max_queries, cand_capacity, nq, top_k,
the tree's mean_diffs, and the placement: whole, 2 / 3 / 5 shards, odd and even num_codes prefixes (also sharded), parts at
global_offset 1 000 000 (a multiple of 32), 1 000 003 and 12 345 678 (not), as the global tail (N even and odd) or not.

Deliberately out: the flat / exact handles (dpq_flat_* have their own edge grids in test_exact_*.py), the asynchronous
pipelines (they have no filtered form), and K = 1 (every code is the same code: nothing for a filter or a radius to cut).

The CPU tests pin the references on a hand-written case, check that the table is the one described here, and that no case
is vacuous (on the references alone)."""
import numpy as np
import pytest

import _option_matrix as om

f32 = np.float32


# ---- CPU ------------------------------------------------------------------------------------------------------------

def _has(**want):
    def match(c):
        return all((c[k] in v) if isinstance(v, (set, tuple, list)) else c[k] == v for k, v in want.items())
    return [c for c in om.TABLE if match(c)]


def _unaligned_part(c):
    return c["global_n"] and c["offset"] % 32 != 0


def _is_tail(c):
    return c["global_n"] and c["offset"] + c["n"] == c["global_n"]


def test_table_is_what_the_issue_says():
    T = om.TABLE
    assert 40 <= len(T) <= 60
    ids = [om.case_id(c) for c in T]
    assert len(set(ids)) == len(ids)
    assert om._build_table() == T                                     # seeded: the same table every time
    for c in T:
        assert 1 <= c["n"] <= 70001 and 1 <= c["nq"] <= 500
        assert c["k"] < c["n"] or c["n"] == 1
    for name, values in om.AXES.items():
        for v in values:
            if name == "mkd":
                hits = [c for c in T if (c["M"], c["K"], c["Ds"]) == tuple(v)]
            else:
                hits = [c for c in T if c[name] == v]
            assert len(hits) >= 2, "%s = %r occurs in %d cases" % (name, v, len(hits))
    # placements
    for s in (2, 3, 5):
        assert len(_has(shards=s)) >= 2, s
    assert len([c for c in T if c["shards"] == 1 and not c["num_codes"] and not c["global_n"]]) >= 2
    for parity in (0, 1):
        assert len([c for c in T if c["num_codes"] and c["num_codes"] % 2 == parity]) >= 2, parity
        assert [c for c in T if c["num_codes"] and c["num_codes"] % 2 == parity and c["shards"] == 2], parity
    for off in om.OFFSETS:
        assert len(_has(offset=off)) >= 2, off
    tails = [c for c in T if _is_tail(c)]
    assert {c["global_n"] % 2 for c in tails} == {0, 1}
    assert [c for c in T if c["global_n"] and not _is_tail(c)]
    # the mandatory cases
    assert [c for c in T if _unaligned_part(c) and _is_tail(c) and c["global_n"] % 2 == 0]
    assert [c for c in T if _unaligned_part(c) and not _is_tail(c)]
    assert [c for c in T if _unaligned_part(c) and c["n"] == 40000 and c["boot"] == 1]
    for n in (1, 65):
        assert [c for c in T if _unaligned_part(c) and c["n"] == n], n
    for n in (1, 65, 4097):
        assert _has(cps=64, n=n), n
    assert _has(cps=1, shards=5, n=257)
    assert [c for c in T if (c["M"], c["K"], c["Ds"]) == (16, 64, 8) and c["bd"] == 37]
    for flags in (64, 192):
        for nq in (1, 4):
            assert [c for c in _has(flags=flags, nq=nq, boot=1) if c["shards"] > 1 and c["n"] // c["shards"] >= 16384], (flags, nq)
    assert [c for c in _has(cap=64) if c["frac"] == 0.005]
    assert [c for c in T if c["num_codes"] and c["num_codes"] % 2 == 0 and c["shards"] > 1]


def test_references_on_a_hand_written_case():
    """Five codes at base 1 000 003 (not a multiple of 32) that end an index of N = 1 000 008 codes (even): the last is
    reported as N."""
    base, N = 1_000_003, 1_000_008
    d = np.array([4.0, 1.0, 3.0, 1.0, 2.0], dtype=f32)
    assert om.reported_ids(np.arange(5), base, N).tolist() == [1000003, 1000004, 1000005, 1000006, 1000008]
    assert om.positions_of([1000008, 1000003, 1000006], base, N).tolist() == [4, 0, 3]
    assert om.reported_ids(np.arange(5), base, 2_000_000).tolist() == [1000003, 1000004, 1000005, 1000006, 1000007]   # not the tail

    def mask(n_bits, ids):
        m = np.zeros(n_bits, dtype=bool)
        m[ids] = True
        return m

    def rows(got, ids, dists):
        assert got[0].dtype == np.int32 and got[1].dtype == f32
        assert got[0].tolist() == ids and got[1].tolist() == dists, got

    inf = float("inf")
    # bit N set, bit N - 1 clear: the last node is eligible under id N
    a = mask(N + 1, [1000003, 1000006, N])
    rows(om.expected_topk(d, a, 4, base, N), [1000006, 1000008, 1000003, -1], [1.0, 2.0, 4.0, inf])
    rows(om.expected_topk(d, a, 2, base, N), [1000006, 1000008], [1.0, 2.0])
    # the opposite: bit N - 1 governs nothing; the tie at 1.0 goes by id
    b = mask(N + 1, [1000004, 1000006, N - 1])
    rows(om.expected_topk(d, b, 3, base, N), [1000004, 1000006, -1], [1.0, 1.0, inf])
    rows(om.expected_topk(d, b, 1, base, N), [1000004], [1.0])
    assert len(om.eligible(b, 5, base, N)[0]) == 2
    # n_bits shorter than the id range: ids at or beyond it are not allowed
    rows(om.expected_topk(d, np.ones(1000005, dtype=bool), 3, base, N), [1000004, 1000003, -1], [1.0, 4.0, inf])
    rows(om.expected_topk(d, np.ones(0, dtype=bool), 2, base, N), [-1, -1], [inf, inf])
    # a shard's own answer: nodes [1 000 005, 1 000 008)
    ones = np.ones(N + 40, dtype=bool)
    rows(om.expected_topk(d, ones, 2, base, N, 1000005, 1000008), [1000006, 1000008], [1.0, 2.0])
    rows(om.expected_topk(d, ones, 2, base, N, 1000003, 1000005), [1000004, 1000003], [1.0, 4.0])
    # the same five codes in the middle of a larger index: no id N
    rows(om.expected_topk(d, ones, 5, base, 2_000_000), [1000004, 1000006, 1000007, 1000005, 1000003], [1.0, 1.0, 2.0, 3.0, 4.0])
    # range lists: a radius exactly equal to a distance excludes it
    rows(om.expected_range(d, f32(3.0), base, N), [1000004, 1000006, 1000008], [1.0, 1.0, 2.0])
    rows(om.expected_range(d, np.nextafter(f32(3.0), f32(inf)), base, N), [1000004, 1000006, 1000008, 1000005], [1.0, 1.0, 2.0, 3.0])
    rows(om.expected_range(d, f32(0.0), base, N), [], [])
    rows(om.expected_range(d, f32(1.0), base, N), [], [])
    rows(om.expected_range(d, f32(inf), base, N), [1000004, 1000006, 1000008, 1000005, 1000003], [1.0, 1.0, 2.0, 3.0, 4.0])
    rows(om.expected_range(d, f32(3.0), base, N, 1000005, 1000008), [1000006, 1000008], [1.0, 2.0])
    # the radius kinds on five distances: rank min(9, (5 - 1) // 2) = 2 stands in for "the 10th"
    assert [float(om.radius_menu(d, i)) for i in (0, 1, 2, 4, 5)] == [0.0, 0.5, 2.0, 2.0, inf]
    assert om.radius_menu(d, 3) == np.nextafter(f32(2.0), f32(inf))
    twenty = np.arange(20, 0, -1).astype(f32)
    assert float(om.radius_menu(twenty, 2)) == 10.0                    # from 20 codes on: the 10th distance itself


def test_no_case_is_vacuous(oracle, lib):
    """On the references alone: in every case some filter allows fewer codes than top_k (padding) and some more, and
    some range list is empty, some holds every code of its handle, and some is cut at an interior radius that equals
    no distance of the handle.  (n = 1: neither "more" nor "interior" exists.)"""
    for c in om.TABLE:
        what = om.case_id(c)
        inp = om.build_inputs(c)
        alld = om.oracle_distances(oracle, c, inp)
        masks, radii = om.make_masks(c), om.radii_calls(c, alld)
        k, base, N, ne = om.call_k(c), c["offset"], om.n_total(c), om.n_eff(c)
        bounds = om.handle_bounds(c, inp)
        assert bounds[0][0] == base and bounds[-1][1] == base + ne and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:])), what
        assert all(lo < hi for lo, hi in bounds), "%s: an empty shard" % what
        allowed = [len(om.eligible(m, ne, base, N, lo, hi)[0]) for lo, hi in bounds for _, m in masks]
        kinds = set()
        for lo, hi in bounds:
            d = alld[:, lo - base:hi - base]
            for r in radii:
                cnt = (d < r[:, None]).sum(axis=1)
                tie = (d == r[:, None]).any(axis=1)
                kinds |= {"empty"} if (cnt == 0).any() else set()
                kinds |= {"all"} if (cnt == hi - lo).any() else set()
                kinds |= {"interior"} if ((cnt > 0) & (cnt < hi - lo) & ~tie).any() else set()
        assert min(allowed) < k, what
        assert {"empty", "all"} <= kinds, (what, kinds)
        if ne > 1:
            assert max(allowed) > k, what
            assert "interior" in kinds, what
        n_bits = [len(m) for _, m in masks]
        id_end = int(om.reported_ids(np.arange(ne), base, N).max()) + 1
        assert n_bits[0] > id_end and n_bits[1] < id_end and n_bits[2] == id_end, what
        assert n_bits[1] % 32 != 0 or n_bits[1] == 0, what


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("case", om.TABLE, ids=om.case_id)
def test_option_matrix(gpu, oracle, case):
    om.run_case(gpu, oracle, case)
