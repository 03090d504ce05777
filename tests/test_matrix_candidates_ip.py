"""Candidate search (dpq_candidate_*) and inner-product search (dpq_query_batch_ip) crossed with every dpq_open_opts field
of the option matrix, handles whose ids lie just inside the int32 range, and calls that meet batches in flight.

tests/_matrix_candidates_ip.py holds the candidate lists, the references and the call sequences; the cases are om.TABLE
of tests/_option_matrix.py (one pytest id per case, `-k <id>` reproduces it) and the hand-written MC.TOP_CASES / MC.TOP_PAIR.
Every comparison is strict, ids and float bits, against plain numpy over the oracle's per-code distances (L2) or over the
restated inner-product tables (gaps): the orders are the header's, (distance bits, id) and (gap bits, id), keys once,
padding -1 / +inf (scores -inf).

Per handle of a case -- the whole index, every shard, a prefix, a part -- the candidate test calls candidate_search over
the wide list at top-1, top-k and, where n_cand <= 2048, top-n_cand; over the few list (fewer valid ids than top_k, query
0 none); candidate_distances; candidate_search_tables (on the first handle also before set_codebook); the handle's own
query_batch ids as the list; the device forms; a list with an id that names no node (DPQ_ERR_ARG from the host and the
device form, the next answer unchanged); and query_batch again.  Sharded cases merge the wide answers.  The
inner-product test calls query_batch_ip, the same under the case's random mask, and the device form with gaps and bias;
sharded cases merge the gaps, score once and compare the biases.

Exact tables: the inner-product tables of EVERY case here (om.TABLE, MC.TOP_CASES, MC.TOP_PAIR and the two cases of the
in-flight tests) are exact in the sense of tests/_numeric_edges.py's table_units, so no case needs the comparison against
query_batch_tables: test_which_ip_tables_are_exact computes the list (it is empty) without a GPU.
"""
import numpy as np
import pytest

import _candidates_restatement as C
import _matrix_candidates_ip as MC
import _numeric_edges as ne
import _option_matrix as om
import _tables_restatement as T

f32 = np.float32
IN_FLIGHT = [om.make_case(4097, bd=1, nq=65, k=10, seed=301), om.make_case(17001, boot=1, flags=64, nq=65, k=10, seed=302)]


def _all_cases():
    return om.TABLE + MC.TOP_CASES + MC.TOP_PAIR + IN_FLIGHT


def pair_inputs(oracle):
    """(inps, joint inp, alld [nq][8192]) of MC.TOP_PAIR: two payloads, one codebook, one set of queries."""
    inps = [om.build_inputs(c) for c in MC.TOP_PAIR]
    assert np.array_equal(inps[0]["cb"], inps[1]["cb"]) and np.array_equal(inps[0]["qs"], inps[1]["qs"])
    joint = dict(cb=inps[0]["cb"], qs=inps[0]["qs"], codes=np.concatenate([i["codes"] for i in inps]))
    alld = np.concatenate([om.oracle_distances(oracle, c, i) for c, i in zip(MC.TOP_PAIR, inps)], axis=1)
    return inps, joint, alld


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_no_list_is_vacuous(lib):
    """On the references alone, for every case: no entry names no node; some handle's wide list holds more than top_k
    distinct local ids (n = 1 cannot) and every few list fewer; a sharded case or a part has a real id that some handle
    skips; a case that holds the even-N tail lists N on the handle that holds it."""
    for c in om.TABLE + MC.TOP_CASES:
        what = om.case_id(c)
        geo = MC.geometry(c)
        lists = MC.make_lists(c)
        assert lists["wide"].shape[1] <= 4810 and lists["few"].shape[1] == om.call_k(c) + 2, what
        assert lists["wide"].shape[1] >= om.call_k(c), what
        facts = MC.list_facts(c, om.handle_bounds(c, om.build_inputs(c)), lists)
        assert facts["none"] == 0, what
        assert facts["few_distinct"] < om.call_k(c), what
        if geo[1] > 1:
            assert facts["wide_distinct"] > om.call_k(c), what
        if c["shards"] > 1 or c["offset"]:
            assert facts["skipped"], what
        if MC.holds_even_tail(geo):
            assert facts["tail_listed"], what
        bad = lists["wide"].copy()
        bad[c["nq"] // 2, 0] = MC.bad_id(geo)
        assert (C.classify(bad, **MC.id_rules(geo[0], geo[0] + geo[1], geo[2]))[0] == C.NONE).sum() == 1, what
    lists = MC.make_lists(MC.TOP_PAIR[0], MC.PAIR_GEO)
    lo, mid, hi = MC.PAIR_GEO[0], MC.TOP_PAIR[1]["offset"], MC.TOP
    facts = MC.list_facts(MC.TOP_PAIR[0], [(lo, mid), (mid, hi)], lists, MC.PAIR_GEO)
    assert facts["none"] == 0 and facts["skipped"] and facts["tail_listed"] and facts["wide_distinct"] > 100 > facts["few_distinct"]


def test_which_ip_tables_are_exact():
    """The cases with a table that is not exact (the module docstring names them: none).  table_is_exact is numpy's
    reading of ne.table_units; the two are compared on the first table of every case and on tables made to fail."""
    not_exact = []
    for c in _all_cases():
        inp = om.build_inputs(c)
        e = T.ip_tables(inp["cb"], inp["qs"])[2]
        assert np.all(np.isfinite(e)) and np.all(e >= 0)
        if not all(MC.table_is_exact(t) for t in e):
            not_exact.append(om.case_id(c))
        ne.table_units([[ne.from_f32(v) for v in row] for row in e[0]])          # asserts exactness itself
        assert MC.table_is_exact(e[0])
    assert not_exact == []
    wide = np.ones((8, 4), dtype=f32)
    wide[3, 2] = f32(2.0 ** 60)
    for t, exact in ((wide, False), (np.ones((8, 4), dtype=f32), True), (np.zeros((8, 4), dtype=f32), True)):
        assert MC.table_is_exact(t) == exact
        try:
            ne.table_units([[ne.from_f32(v) for v in row] for row in t])
            assert exact
        except AssertionError:
            assert not exact


def test_top_cases_lie_at_the_top_of_the_id_range():
    top = 0
    for c in MC.TOP_CASES + MC.TOP_PAIR:
        base, n, N = MC.geometry(c)
        rep = om.reported_ids(np.arange(n), base, N)
        assert rep.max() > 2 ** 30 and rep.max() < 2 ** 31, om.case_id(c)
        assert N <= MC.TOP and base + n <= N
        if base + n == N:
            assert rep.max() == (N if N % 2 == 0 else N - 1), om.case_id(c)       # an even-N tail reports N itself
        top = max(top, base + n)
    # the open check refuses n_codes, global_n_codes and global_offset + n_codes from INT32_MAX on (open_from_payload)
    assert top == MC.TOP == np.iinfo(np.int32).max - 1
    assert sorted(c["global_n"] for c in MC.TOP_CASES if c["offset"] + c["n"] == c["global_n"]) == [MC.TOP - 1] + [MC.TOP] * 5
    crossing = MC.TOP_CASES[3]
    assert crossing["offset"] < 2 ** 30 < crossing["offset"] + crossing["n"]
    assert MC.TOP_PAIR[0]["offset"] + 4095 == MC.TOP_PAIR[1]["offset"] and MC.TOP_PAIR[1]["offset"] + 4097 == MC.TOP


def test_references_on_a_hand_written_case_at_the_top():
    """Five codes at base 2 147 483 641 that end an index of N = 2 147 483 646 codes (even): the last is reported as N."""
    base, N = 2147483641, 2147483646
    L, S, X = C.LOCAL, C.SKIP, C.NONE
    inf, nan = float("inf"), float("nan")
    geo = dict(id_base=base, n_local=5, n_total=N, even_rule=True)
    d = np.array([4.0, 1.0, 3.0, 1.0, 2.0], dtype=f32)
    assert om.reported_ids(np.arange(5), base, N).tolist() == [2147483641, 2147483642, 2147483643, 2147483644, 2147483646]
    cand = [2147483646, 2147483645, 2147483640, -1, 2147483642, 2147483644, 2147483642, 2147483641]
    cls, local = C.classify(cand, **geo)
    assert cls.tolist() == [L, X, S, S, L, L, L, L] and local.tolist() == [4, -1, -1, -1, 1, 3, 1, 0]
    with pytest.raises(ValueError):
        C.search_row(d, cand, 3, **geo)
    good = [2147483646, 2147483640, -1, 2147483642, 2147483644, 2147483642, 2147483641]
    got = C.candidate_distances(d, good, **geo)
    assert np.isnan(got).tolist() == [False, True, True, False, False, False, False]
    assert got[[0, 3, 4, 5, 6]].tolist() == [2.0, 1.0, 1.0, 1.0, 4.0] and np.all(MC.bits(got[[1, 2]]) == 0x7FC00000)
    ids, dist = C.search_row(d, good, 3, **geo)
    assert ids.dtype == np.int32 and ids.tolist() == [2147483642, 2147483644, 2147483646] and dist.tolist() == [1.0, 1.0, 2.0]
    ids, dist = C.search_row(d, good, 5, **geo)
    assert ids.tolist() == [2147483642, 2147483644, 2147483646, 2147483641, -1] and dist.tolist() == [1.0, 1.0, 2.0, 4.0, inf]
    # the handle below it, nodes [base - 5, base): everything above is another handle's, N included
    below = dict(id_base=base - 5, n_local=5, n_total=N, even_rule=True)
    assert C.classify(good, **below)[0].tolist() == [S, L, S, S, S, S, S]
    assert C.search_row(d, good, 2, **below)[0].tolist() == [2147483640, -1]
    # the inner-product row over hand-given gaps, bias 1.5
    g = np.array([0.5, 0.0, 0.25, 0.0, 0.25], dtype=f32)
    pos = np.arange(5)
    rep = om.reported_ids(pos, base, N)
    ids, gaps = om.topk_row(g, pos, rep, 4)
    assert ids.tolist() == [2147483642, 2147483644, 2147483643, 2147483646] and gaps.tolist() == [0.0, 0.0, 0.25, 0.25]
    assert T.ip_scores([1.5], gaps[None], ids[None]).tolist() == [[1.5, 1.5, 1.25, 1.25]]
    ids, gaps = om.topk_row(g, pos[[0, 4]], rep[[0, 4]], 3)
    assert ids.tolist() == [2147483646, 2147483641, -1] and gaps.tolist() == [0.25, 0.5, inf]
    assert T.ip_scores([1.5], gaps[None], ids[None]).tolist() == [[1.25, 1.0, -inf]]
    assert MC.bad_id((base, 5, N)) == N - 1 and MC.bad_id((base - 5, 5, N)) == N + 1 and MC.bad_id((base, 4, N - 1)) == N - 1


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("case", om.TABLE, ids=om.case_id)
def test_candidate_search_over_the_matrix(gpu, oracle, case):
    inp = om.build_inputs(case)
    MC.run_candidates(gpu, case, inp, om.oracle_distances(oracle, case, inp), MC.make_lists(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", om.TABLE, ids=om.case_id)
def test_ip_search_over_the_matrix(gpu, case):
    inp = om.build_inputs(case)
    MC.run_ip(gpu, case, inp, MC.ip_reference(case, inp), dict(om.make_masks(case))["random"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", MC.TOP_CASES, ids=om.case_id)
def test_handles_at_the_top_of_the_id_range(gpu, oracle, case):
    inp = om.build_inputs(case)
    alld = om.oracle_distances(oracle, case, inp)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], case["n"], case["M"], case["K"], **om.open_kwargs(case)) as idx:
        MC.top_calls(gpu, idx, case, inp, alld, MC.ip_reference(case, inp), MC.make_lists(case), om.case_id(case))


@pytest.mark.gpu
def test_two_adjacent_parts_at_the_top_of_the_id_range(gpu, oracle):
    """4095 + 4097 codes that end an index of 2^31 - 2: both parts take the same lists, and the merged answers -- on the
    host and on the device -- are the two-part expectation, every id unchanged."""
    import torch
    inps, joint, alld = pair_inputs(oracle)
    c0 = MC.TOP_PAIR[0]
    base, n, N = geo = MC.PAIR_GEO
    nq, k = c0["nq"], om.call_k(c0)
    ref = MC.ip_reference(dict(c0, n=n), joint)
    lists = MC.make_lists(c0, geo)
    # the ids on both sides of the seam and at both ends, top_k = n_cand: every one of them comes back, N among them
    mid = MC.TOP_PAIR[1]["offset"]
    seam = np.tile(np.array([N, base, mid - 1, -1, mid, mid + 1, N - 2, base + 1], dtype=np.int32), (nq, 1))
    parts = []
    for c, inp in zip(MC.TOP_PAIR, inps):
        with gpu.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c)) as idx:
            parts.append(MC.top_calls(gpu, idx, c, inp, alld, ref, lists, "pair, part at %d" % c["offset"], geo))
            parts[-1]["seam"] = idx.candidate_search(inp["qs"], seam, seam.shape[1])
    pos = np.arange(n)
    rep = om.reported_ids(pos, base, N)
    r = MC.id_rules(base, base + n, N)
    want = dict(first=[om.topk_row(alld[q], pos, rep, k) for q in range(nq)],
                wide=[C.search_row(alld[q], lists["wide"][q], k, **r) for q in range(nq)],
                seam=[C.search_row(alld[q], seam[q], seam.shape[1], **r) for q in range(nq)])
    for name in ("first", "wide", "seam"):
        ids, d = np.stack([p[name][0] for p in parts]), np.stack([p[name][1] for p in parts])
        om._rows_equal(gpu.merge_topk_host(ids, d), want[name], "pair, %s merged on the host" % name)
        ti, td = gpu.merge_topk_torch(torch.from_numpy(ids).cuda(), torch.from_numpy(d).cuda())
        om._rows_equal((ti.cpu().numpy(), td.cpu().numpy()), want[name], "pair, %s merged on the device" % name)
    assert all(sorted(w[0].tolist()) == [-1, base, base + 1, mid - 1, mid, mid + 1, N - 2, N] for w in want["seam"])
    assert all(w[0].min() > 2 ** 30 for w in want["first"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", IN_FLIGHT, ids=om.case_id)
def test_calls_meet_batches_in_flight(gpu, oracle, case):
    """Two laned batches (65 queries, 1 query) are enqueued and NOT finished; candidate_search, query_batch_ip and
    candidate_distances settle them on their own way in.  All five answers are the synchronous references'."""
    import torch
    c = case
    inp = om.build_inputs(c)
    alld = om.oracle_distances(oracle, c, inp)
    ref = MC.ip_reference(c, inp)
    assert ref["exact"].all()
    wide = MC.make_lists(c)["wide"]
    n, k, qs = c["n"], c["k"], inp["qs"]
    pos = np.arange(n)
    r = MC.id_rules(0, n, n)
    with gpu.DeltaPQIndex.open_memory(inp["payload"], n, c["M"], c["K"], **om.open_kwargs(c)) as idx:
        idx.set_codebook(inp["cb"])
        t_q, t_one, t_w = torch.from_numpy(qs).cuda(), torch.from_numpy(qs[7:8].copy()).cuda(), torch.from_numpy(wide).cuda()
        many = idx.query_batch_torch(t_q, k, wait=False)
        one = idx.query_batch_torch(t_one, k, wait=False)
        cand = idx.candidate_search(qs, wide, k)
        ip = idx.query_batch_ip(qs, k)
        dist = idx.candidate_distances_torch(t_q, t_w)
        assert idx.finish() == 0
        torch.cuda.synchronize()
        want = [om.topk_row(alld[q], pos, pos, k) for q in range(c["nq"])]
        om._rows_equal((many[0].cpu().numpy(), many[1].cpu().numpy()), want, "the batch of 65 in flight")
        om._rows_equal((one[0].cpu().numpy(), one[1].cpu().numpy()), want[7:8], "the batch of 1 in flight")
        om._rows_equal(cand, [C.search_row(alld[q], wide[q], k, **r) for q in range(c["nq"])], "candidate_search")
        MC.check_ip(ip, MC.ip_rows(ref["g"], ref["B"], pos, pos, k), ref["B"], "query_batch_ip")
        want_d = np.stack([C.candidate_distances(alld[q], wide[q], **r) for q in range(c["nq"])])
        assert np.array_equal(MC.bits(dist.cpu().numpy()), MC.bits(want_d)), "candidate_distances, device form"
        assert MC.same(idx.query_batch(qs, k), (many[0].cpu().numpy(), many[1].cpu().numpy()))
