"""IVF search (dpq_ivf_*) crossed with every dpq_open_opts field of the option matrix, with handles whose ids lie just
inside the int32 range, and with batches in flight.

tests/_matrix_ivf.py holds the labels, the probes, the centroids, the references and the call sequence; the cases are
om.TABLE of tests/_option_matrix.py and MC.TOP_CASES / MC.TOP_PAIR of tests/_matrix_candidates_ip.py, one pytest id per
case (`-k <id>` reproduces it).  Every comparison is strict, ids and float bits, against tests/_ivf_restatement.py over the
oracle's per-code distances: the order is the header's (distance bits, id), a list named twice counts once, padding is
-1 / +inf.

Per handle of a case -- the whole index, every shard, a prefix, a part, each half of the pair -- the lists from host labels
and from a device tensor, their counts, search_probes at top-1, at the case's top_k and at a top_k that pads, the device
form, every node labelled and every list probed (query_batch's answer wherever top_k fits the handle), the lists by
centroids with probe and search, and query_batch again.  Sharded cases and the pair merge the answers.

test_no_ivf_case_is_vacuous runs on the references alone.  Its conditions hold for every case they can hold for; the
cases for which one cannot hold are worked out there from the numbers of the case, each with its reason:
 * no list can be empty on one handle and not on another where the index has at most three codes or one list only (a
   single list is empty only on a handle without a labelled node);
 * no row can pad where nprobe < nlist and even the smallest probed union holds 2048 codes or more (top_k ends there).
"""
import numpy as np
import pytest

import _ivf_restatement as R
import _matrix_candidates_ip as MC
import _matrix_ivf as MI
import _option_matrix as om


def pair_inputs(oracle):
    """(inps, joint inp, alld [nq][8192]) of MC.TOP_PAIR: two payloads, one codebook, one set of queries."""
    inps = [om.build_inputs(c) for c in MC.TOP_PAIR]
    assert np.array_equal(inps[0]["cb"], inps[1]["cb"]) and np.array_equal(inps[0]["qs"], inps[1]["qs"])
    joint = dict(cb=inps[0]["cb"], qs=inps[0]["qs"], codes=np.concatenate([i["codes"] for i in inps]))
    alld = np.concatenate([om.oracle_distances(oracle, c, i) for c, i in zip(MC.TOP_PAIR, inps)], axis=1)
    return inps, joint, alld


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_no_ivf_case_is_vacuous(lib):
    cannot_be_uneven, cannot_pad, powers_of_two = [], [], set()
    pair_bounds = [(MC.PAIR_GEO[0], MC.TOP_PAIR[1]["offset"]), (MC.TOP_PAIR[1]["offset"], MC.TOP)]
    for c in MI.CASES + [MI.PAIR]:
        what = om.case_id(c)
        geo = MC.PAIR_GEO if c is MI.PAIR else MC.geometry(c)
        n = geo[1]
        plan = MI.make_plan(c, geo)
        bounds = pair_bounds if c is MI.PAIR else om.handle_bounds(c, om.build_inputs(c))
        f = MI.plan_facts(c, plan, bounds, geo)
        nlist, nprobe, ks = plan["nlist"], plan["nprobe"], plan["ks"]
        assert 1 <= nprobe <= nlist <= max(1, n) and plan["labels"][-1] >= 0 and np.all(plan["probes"][:, 0] == plan["last"]), what
        assert plan["labels"].max() < nlist and plan["full"].min() >= 0 and plan["full"].max() < nlist, what
        assert 1 in ks and plan["k"] in ks and max(ks) <= 2048, what
        if nprobe >= 3:
            assert f["minus_one"] and (f["repeat"] or (c["nq"] == 1 and nprobe == 3)), what
        if n >= 20:
            assert f["unassigned"] > 0, what + ": no unassigned node"
            assert f["sizes"].max() > min(ks), what + ": no probed union is larger than a top_k"
            if nprobe < nlist:
                if f["sizes"].min() >= 2048:
                    cannot_pad.append(what)                  # top_k <= 2048 <= every union
                else:
                    assert f["sizes"].min() < max(ks), what + ": no probed union is smaller than a top_k"
        if len(bounds) > 1:
            if n <= 3 or nlist == 1:                         # (one list cannot be empty where a labelled node is)
                cannot_be_uneven.append((what, n, nlist))
            else:
                assert f["uneven"], what + ": no list is empty on one handle and not on another"
        if MC.holds_even_tail(geo):
            assert f["tail_probed"], what + ": the id N is in no probed list"
        if f["unassigned"] and nlist & (nlist - 1) == 0:
            powers_of_two.add(nlist)
    assert len(powers_of_two) >= 3, "unassigned nodes meet the powers of two %s only" % sorted(powers_of_two)
    # the cases a condition cannot hold for, by the case's own numbers
    assert all(n <= 3 or nlist == 1 for _, n, nlist in cannot_be_uneven)
    print("cannot be uneven: %s\ncannot pad: %s" % (cannot_be_uneven, cannot_pad))
    assert len(cannot_pad) <= 2 and len(cannot_be_uneven) <= 3, (cannot_pad, cannot_be_uneven)


def test_the_plan_on_a_hand_checked_case():
    """The rules of make_plan, read off one case: n = 4097, a part that ends an even-N index."""
    c = next(c for c in MI.CASES if c["n"] == 4097 and c["seed"] == 101)
    base, n, N = MC.geometry(c)
    assert MC.holds_even_tail((base, n, N))
    plan = MI.make_plan(c)
    off, ids = MI.handle_lists(plan["labels"], plan["nlist"], base, base + n, (base, n, N))
    assert ids.max() == N and N - 1 not in ids and len(ids) == (plan["labels"] >= 0).sum()
    assert np.array_equal(np.sort(ids), np.sort(om.reported_ids(np.flatnonzero(plan["labels"] >= 0), base, N)))
    assert N in R.union(off, ids, plan["probes"][0])
    assert MI.union_sizes(plan["labels"], plan["nlist"], plan["probes"])[0] == len(R.union(off, ids, plan["probes"][0]))
    cb = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2)
    assert MI.reconstruct(cb, np.array([[2, 0], [1, 1]])).tolist() == [[4, 5, 6, 7], [2, 3, 8, 9]]


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("case", MI.CASES, ids=om.case_id)
def test_ivf_search_over_the_matrix(gpu, oracle, case):
    inp = om.build_inputs(case)
    MI.run_case(gpu, case, inp, om.oracle_distances(oracle, case, inp), MI.make_plan(case))


@pytest.mark.gpu
def test_two_adjacent_parts_at_the_top_of_the_id_range(gpu, oracle):
    """4095 + 4097 codes that end an index of 2^31 - 2: both parts take their slices of one label array and the same
    probes and centroids; the merged answers -- on the host and on the device -- are the two-part expectation."""
    import torch
    inps, joint, alld = pair_inputs(oracle)
    geo = MC.PAIR_GEO
    plan = MI.make_plan(MI.PAIR, geo)
    cents = MI.reconstruct(joint["cb"], joint["codes"][plan["cent_rows"]])
    parts = []
    for c, inp in zip(MC.TOP_PAIR, inps):
        with gpu.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c)) as idx:
            idx.set_codebook(inp["cb"])
            parts.append(MI.ivf_calls(gpu, idx, MI.PAIR, joint, alld, plan, "pair, part at %d" % c["offset"], geo, cents))
    whole = MI.whole_reference(MI.PAIR, joint, alld, plan, geo)
    for name in ("probes", "cents"):
        ids, d = np.stack([p[name][0] for p in parts]), np.stack([p[name][1] for p in parts])
        om._rows_equal(gpu.merge_topk_host(ids, d), whole[name], "pair, %s merged on the host" % name)
        ti, td = gpu.merge_topk_torch(torch.from_numpy(ids).cuda(), torch.from_numpy(d).cuda())
        om._rows_equal((ti.cpu().numpy(), td.cpu().numpy()), whole[name], "pair, %s merged on the device" % name)
    lists = MI.handle_lists(plan["labels"], plan["nlist"], geo[0], geo[0] + geo[1], geo)
    assert geo[2] in R.union(*lists, plan["probes"][0]) and all(w[0][0] > 2 ** 30 for w in whole["probes"])


def _in_flight(gpu, oracle, c):
    import torch
    inp = om.build_inputs(c)
    alld = om.oracle_distances(oracle, c, inp)
    plan = MI.make_plan(c)
    n, k, qs = c["n"], c["k"], inp["qs"]
    geo = (0, n, n)
    lists = MI.handle_lists(plan["labels"], plan["nlist"], 0, n, geo)
    pos = np.arange(n)
    want_all = [om.topk_row(alld[q], pos, pos, k) for q in range(c["nq"])]
    want = MI.handle_search(alld, lists, plan["probes"], k, 0, n, geo)
    idx = gpu.DeltaPQIndex.open_memory(inp["payload"], n, c["M"], c["K"], **om.open_kwargs(c))
    idx.set_codebook(inp["cb"])
    t_q, t_one = torch.from_numpy(qs).cuda(), torch.from_numpy(qs[7:8].copy()).cuda()
    return idx, plan, lists, qs, k, t_q, t_one, want_all, want


@pytest.mark.gpu
@pytest.mark.parametrize("case", MI.IN_FLIGHT, ids=om.case_id)
def test_from_labels_meets_batches_in_flight(gpu, oracle, case):
    """Two laned batches (65 queries, 1 query) are enqueued and NOT finished; IVF.from_labels settles them on its way in."""
    import torch
    idx, plan, lists, qs, k, t_q, t_one, want_all, want = _in_flight(gpu, oracle, case)
    with idx:
        many = idx.query_batch_torch(t_q, k, wait=False)
        one = idx.query_batch_torch(t_one, k, wait=False)
        with gpu.IVF.from_labels(idx, plan["labels"], plan["nlist"]) as ivf:
            got_lists = ivf.lists()
            got = ivf.search_probes(qs, plan["probes"], k)
        assert idx.finish() == 0
        torch.cuda.synchronize()
        om._rows_equal((many[0].cpu().numpy(), many[1].cpu().numpy()), want_all, "the batch of 65 in flight")
        om._rows_equal((one[0].cpu().numpy(), one[1].cpu().numpy()), want_all[7:8], "the batch of 1 in flight")
        assert np.array_equal(got_lists[0], lists[0]) and np.array_equal(got_lists[1], lists[1])
        om._rows_equal(got, want, "search_probes on lists made while batches were in flight")
        assert MC.same(idx.query_batch(qs, k), (many[0].cpu().numpy(), many[1].cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", MI.IN_FLIGHT, ids=om.case_id)
def test_search_probes_meets_batches_in_flight(gpu, oracle, case):
    """The lists exist; two laned batches are enqueued and NOT finished; search_probes and its device form settle them."""
    import torch
    idx, plan, lists, qs, k, t_q, t_one, want_all, want = _in_flight(gpu, oracle, case)
    with idx, gpu.IVF.from_labels(idx, plan["labels"], plan["nlist"]) as ivf:
        t_p = torch.from_numpy(plan["probes"]).cuda()
        many = idx.query_batch_torch(t_q, k, wait=False)
        one = idx.query_batch_torch(t_one, k, wait=False)
        got = ivf.search_probes(qs, plan["probes"], k)
        again = idx.query_batch_torch(t_q, k, wait=False)
        dev = ivf.search_probes_torch(t_q, t_p, k)
        assert idx.finish() == 0
        torch.cuda.synchronize()
        om._rows_equal((many[0].cpu().numpy(), many[1].cpu().numpy()), want_all, "the batch of 65 in flight")
        om._rows_equal((one[0].cpu().numpy(), one[1].cpu().numpy()), want_all[7:8], "the batch of 1 in flight")
        om._rows_equal((again[0].cpu().numpy(), again[1].cpu().numpy()), want_all, "the second batch of 65 in flight")
        om._rows_equal(got, want, "search_probes")
        om._rows_equal((dev[0].cpu().numpy(), dev[1].cpu().numpy()), want, "search_probes, device form")
        assert MC.same(idx.query_batch(qs, k), (many[0].cpu().numpy(), many[1].cpu().numpy()))
