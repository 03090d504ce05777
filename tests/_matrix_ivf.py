"""IVF search crossed with the option matrix of tests/_option_matrix.py and with the handles at the top of the id range of
tests/_matrix_candidates_ip.py: the labels, the probes, the centroids, the references and the call sequence of
tests/test_matrix_ivf.py.  No tests in here, and nothing but numpy.

A case's plan (make_plan) is seeded from c["seed"] + 7 and depends on nothing else: nlist and nprobe come round by the
case's place in CASES, the labels cover every code the case's handles hold together (a handle takes its own slice), the
probes are the same for every handle of the case.  References: tests/_ivf_restatement.py over the oracle's per-code
distances, with the id rules of the handle.  Every comparison is strict: ids and float bits, padding -1 / +inf.

Choices the issue leaves open, and why:
 * nlist is NLISTS[i % 6] and nprobe NPROBES[(i + i // 6) % 4] for case number i: the second term turns the shorter
   cycle by one place per round of the longer, so every nlist meets every nprobe (i % 6 and i % 4 alone never would).
 * a third top_k beside top-1 and min(call_k, 2048): min(2048, largest probed union + 1).  With one list probed every row
   names the same list (column 0 is the list of the last code), so the case's own top_k pads only by luck; this one pads
   every row wherever the largest union stays below 2048.
 * the row with the -1 is nq // 2 and the row with the repeat is nq - 1 (entry 2 repeats entry 0); a case of one query
   carries both in its one row where nprobe >= 4, and the -1 alone at nprobe = 3.
 * the first code is always in the last code's list: every row probes that list, so every union is larger than top-1.
 * a case of several handles (shards, the pair) keeps one list, the one after the last code's, out of the first nine
   tenths of its nodes (its labels there are drawn again among the other lists) and gives it node n - 2: the first handle
   finds it empty and a later one does not.  One list alone (nlist = 1) cannot be empty on a handle that holds a labelled
   node, so such a case has no such list, like the cases of at most three codes.
 * no start of the two cycles (all 6 x 4 were tried) leaves every condition of test_no_ivf_case_is_vacuous satisfiable for
   every case: a sharded case always meets nlist = 1 somewhere, and a case of many codes meets few lists with fewer probes,
   where even the smallest probed union holds 2048 codes or more and no top_k can pad.  The cycles start at 0; the test
   works out which cases these are from their own numbers and holds their count to what it is today (3 and 2).
 * "every node labelled" is abs(labels) mod nlist: the same as abs(labels) from nlist = 2 on, and list 0 at nlist = 1.
 * the centroids are the reconstructions of min(nlist, 16) codes drawn without replacement; equal codes among them are
   equal centroids, whose tie the lowest list wins.
"""
import numpy as np

import _ivf_restatement as R
import _matrix_candidates_ip as MC
import _option_matrix as om

NLISTS = [1, 2, 7, 64, 257, 1024]
NPROBES = [1, 3, 8, None]            # None: every list, capped at 1024
MAX_TOP_K, MAX_PROBE, CENTROID_LISTS = 2048, 1024, 16
PAIR = dict(MC.TOP_PAIR[0], n=MC.PAIR_GEO[1])        # the two adjacent parts as one case: its seed, queries and top_k
CASES = om.TABLE + MC.TOP_CASES                       # + PAIR, which has a test of its own
IN_FLIGHT = [om.make_case(4097, bd=1, nq=65, k=10, seed=301), om.make_case(17001, boot=1, flags=64, nq=65, k=10, seed=302)]


def case_number(c):
    if c is PAIR:
        return len(CASES)
    for i, other in enumerate(CASES + IN_FLIGHT):
        if other is c:
            return i if i < len(CASES) else i + 1
    raise KeyError(om.case_id(c))


def make_plan(c, geo=None):
    """dict(nlist, nprobe, labels int32 [n], full int32 [n], probes int32 [nq][nprobe], everything int32 [nq][min(nlist,
    1024)], ks, cent_rows int64 [nlist4]) of a case; `geo` where the geometry is not the case's own (PAIR)."""
    i = case_number(c)
    rng = np.random.default_rng(c["seed"] + 7)
    base, n, N = MC.geometry(c) if geo is None else geo
    nq = c["nq"]
    nlist = min(NLISTS[i % len(NLISTS)], max(1, n))
    want = NPROBES[(i + i // len(NLISTS)) % len(NPROBES)]
    nprobe = min(nlist if want is None else want, nlist, MAX_PROBE)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    if n >= 20:                                       # a twentieth of the nodes, never the first or the last
        labels[1 + rng.choice(n - 2, size=(n + 10) // 20, replace=False)] = -1
    last = int(labels[-1])
    labels[0] = last                                  # (the last code's list holds two codes from n = 2 on: more than top-1)
    if (c["shards"] > 1 or c is PAIR) and nlist >= 2 and n >= 4:
        # several handles: one list lives in the last tenth of the nodes only, so the first handle finds it empty
        late = (last + 1) % nlist
        early = np.flatnonzero(labels[:n - max(2, n // 10)] == late)
        labels[early] = (late + 1 + rng.integers(0, nlist - 1, size=len(early))) % nlist
        labels[n - 2] = late
    probes = np.empty((nq, nprobe), dtype=np.int32)
    for q in range(nq):
        perm = rng.permutation(nlist)
        perm = np.concatenate([[last], perm[perm != last]])
        probes[q] = perm[:nprobe]
    if nprobe >= 3:
        a, b = nq // 2, nq - 1
        probes[a, 1] = -1
        if b != a:
            probes[b, 2] = probes[b, 0]
        elif nprobe >= 4:
            probes[b, 3] = probes[b, 0]
    width = min(nlist, MAX_PROBE)
    everything = np.stack([rng.permutation(nlist)[:width] for _ in range(nq)]).astype(np.int32)
    cent_rows = np.sort(rng.choice(n, size=min(nlist, CENTROID_LISTS), replace=False))
    sizes = union_sizes(labels, nlist, probes)
    k_case = min(om.call_k(c), MAX_TOP_K)
    ks = sorted({1, k_case, min(MAX_TOP_K, int(sizes.max()) + 1)})
    return dict(nlist=nlist, nprobe=nprobe, labels=labels, full=(np.abs(labels) % nlist).astype(np.int32), probes=probes,
                everything=everything, ks=ks, k=k_case, cent_rows=cent_rows, last=last)


def union_sizes(labels, nlist, probes):
    """int64 [nq]: how many codes each row's distinct, real lists hold."""
    counts = np.bincount(labels[labels >= 0], minlength=nlist)
    return np.array([counts[np.unique(row[row >= 0])].sum() for row in probes], dtype=np.int64)


def reconstruct(cb, codes):
    """float32 [n][M * Ds]: cb[m][codes[., m]] side by side."""
    M = cb.shape[0]
    return np.ascontiguousarray(cb[np.arange(M)[None, :], codes].reshape(len(codes), -1), dtype=np.float32)


def handle_lists(labels, nlist, lo, hi, geo):
    base, _, N = geo
    return R.lists_from_labels(labels[lo - base:hi - base], nlist, node_lo=lo, n_total=N, even_rule=True)


def handle_search(alld, lists, probes, k, lo, hi, geo):
    base, _, N = geo
    return R.search(alld[:, lo - base:hi - base], np.arange(len(probes)), lists[0], lists[1], probes, k, **MC.id_rules(lo, hi, N))


def plan_facts(c, plan, bounds, geo=None):
    """What test_no_ivf_case_is_vacuous asserts, on the references alone."""
    base, n, N = geo = MC.geometry(c) if geo is None else geo
    sizes = union_sizes(plan["labels"], plan["nlist"], plan["probes"])
    per_handle = np.stack([np.bincount(plan["labels"][lo - base:hi - base][plan["labels"][lo - base:hi - base] >= 0],
                                       minlength=plan["nlist"]) for lo, hi in bounds])
    uneven = bool(np.any((per_handle == 0).any(axis=0) & (per_handle > 0).any(axis=0)))
    tail_probed = False
    if MC.holds_even_tail(geo):
        for lo, hi in bounds:
            off, ids = handle_lists(plan["labels"], plan["nlist"], lo, hi, geo)
            tail_probed |= any(N in R.union(off, ids, row) for row in plan["probes"][:2])
    return dict(unassigned=int((plan["labels"] < 0).sum()), sizes=sizes, uneven=uneven, tail_probed=tail_probed,
                minus_one=bool((plan["probes"] < 0).any()),
                repeat=any(len(np.unique(r[r >= 0])) < (r >= 0).sum() for r in plan["probes"]))


# ---- the call sequence -------------------------------------------------------------------------------------------------------

def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def ivf_calls(api, idx, c, inp, alld, plan, what, geo=None, cents=None):
    """The five steps on one open handle with its codebook set.  alld [nq][n] holds the distances of the geometry's codes
    by position, inp["codes"] their codes.  Returns dict(probes=the answer of step 2 at the case's top_k, cents=that of
    step 4)."""
    import torch
    base, n, N = geo = MC.geometry(c) if geo is None else geo
    info = idx.info()
    lo, hi = info["node_lo"], info["node_hi"]
    assert info["n_codes_total"] == N and base <= lo < hi <= base + n, "%s: nodes [%d, %d)" % (what, lo, hi)
    qs, nq, nlist, k = inp["qs"], c["nq"], plan["nlist"], plan["k"]
    labels = np.ascontiguousarray(plan["labels"][lo - base:hi - base])
    probes, everything = plan["probes"], plan["everything"]
    t_q = torch.from_numpy(qs).cuda()
    first = idx.query_batch(qs, min(k, N))
    out = {}
    # 1. lists from labels, host and device
    lists = handle_lists(plan["labels"], nlist, lo, hi, geo)
    with api.IVF.from_labels(idx, labels, nlist) as ivf, api.IVF.from_labels(idx, torch.from_numpy(labels).cuda(), nlist) as dev:
        for name, v in (("host labels", ivf), ("device labels", dev)):
            got = v.lists()
            assert np.array_equal(got[0], lists[0]) and np.array_equal(got[1], lists[1]), "%s: lists from %s" % (what, name)
            inf = v.info()
            lens = np.diff(lists[0])
            assert (inf["nlist"], inf["n_assigned"], inf["n_unassigned"], inf["max_list_len"], inf["has_centroids"]) == \
                (nlist, len(lists[1]), (hi - lo) - len(lists[1]), lens.max(), 0), "%s: info from %s: %s" % (what, name, inf)
        # 2. the named probes
        for kk in plan["ks"]:
            want = handle_search(alld, lists, probes, kk, lo, hi, geo)
            got = ivf.search_probes(qs, probes, kk)
            om._rows_equal(got, want, "%s search_probes top-%d" % (what, kk))
            if kk == k:
                out["probes"] = got
                om._rows_equal(_np(dev.search_probes_torch(t_q, torch.from_numpy(probes).cuda(), kk)), want,
                               "%s search_probes top-%d, device form on the lists from device labels" % (what, kk))
    # 3. every node labelled and every list probed
    full = np.ascontiguousarray(plan["full"][lo - base:hi - base])
    full_lists = handle_lists(plan["full"], nlist, lo, hi, geo)
    with api.IVF.from_labels(idx, full, nlist) as ivf:
        assert ivf.info()["n_unassigned"] == 0 and np.array_equal(ivf.lists()[1], full_lists[1]), what + ": every node labelled"
        got = ivf.search_probes(qs, everything, k)
        om._rows_equal(got, handle_search(alld, full_lists, everything, k, lo, hi, geo), "%s every list probed top-%d" % (what, k))
        if k <= hi - lo and k <= N:
            assert MC.same(got, idx.query_batch(qs, k)), what + ": every list probed differs from query_batch"
    # 4. lists from centroids
    nlist4 = len(plan["cent_rows"])
    nprobe4 = min(plan["nprobe"], nlist4)
    cents = reconstruct(inp["cb"], inp["codes"][plan["cent_rows"]]) if cents is None else cents
    assigned = R.assign(reconstruct(inp["cb"], inp["codes"][lo - base:hi - base]), cents)
    cent_lists = R.lists_from_labels(assigned, nlist4, node_lo=lo, n_total=N, even_rule=True)
    want_l, want_d = R.probe(cents, qs, nprobe4)
    with api.IVF.build(idx, cents) as ivf:
        got = ivf.lists()
        assert np.array_equal(got[0], cent_lists[0]) and np.array_equal(got[1], cent_lists[1]), what + ": lists from centroids"
        assert ivf.info()["has_centroids"] == 1 and ivf.info()["n_unassigned"] == 0, what
        got_l, got_d = ivf.probe(qs, nprobe4)
        assert np.array_equal(got_l, want_l) and np.array_equal(MC.bits(got_d), MC.bits(want_d)), what + ": probe"
        want = handle_search(alld, cent_lists, want_l, k, lo, hi, geo)
        out["cents"] = ivf.search(qs, nprobe4, k)
        om._rows_equal(out["cents"], want, "%s search by centroids, nprobe %d top-%d" % (what, nprobe4, k))
        om._rows_equal(_np(ivf.search_torch(t_q, nprobe4, k)), want, "%s search by centroids, device form" % what)
    # 5. the handle answers as before
    assert MC.same(idx.query_batch(qs, min(k, N)), first), what + ": query_batch changed after the IVF calls"
    return out


def whole_reference(c, inp, alld, plan, geo=None):
    """dict(probes, cents): what the merged answers of steps 2 and 4 must be, over all the case's codes as one handle."""
    base, n, N = geo = MC.geometry(c) if geo is None else geo
    k = plan["k"]
    lists = handle_lists(plan["labels"], plan["nlist"], base, base + n, geo)
    cents = reconstruct(inp["cb"], inp["codes"][plan["cent_rows"]])
    assigned = R.assign(reconstruct(inp["cb"], inp["codes"][:n]), cents)
    cent_lists = R.lists_from_labels(assigned, len(cents), node_lo=base, n_total=N, even_rule=True)
    want_l, _ = R.probe(cents, inp["qs"], min(plan["nprobe"], len(cents)))
    return dict(probes=handle_search(alld, lists, plan["probes"], k, base, base + n, geo),
                cents=handle_search(alld, cent_lists, want_l, k, base, base + n, geo))


def run_case(api, c, inp, alld, plan):
    """Every handle of a case of CASES through ivf_calls; a sharded case's merged answers against the whole case."""
    what = om.case_id(c)
    parts = []
    for rank in range(c["shards"]):
        with api.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c, rank)) as idx:
            idx.set_codebook(inp["cb"])
            parts.append(ivf_calls(api, idx, c, inp, alld, plan, what if c["shards"] == 1 else "%s rank %d" % (what, rank)))
    if c["shards"] > 1:
        whole = whole_reference(c, inp, alld, plan)
        for name in ("probes", "cents"):
            merged = api.merge_topk_host(np.stack([p[name][0] for p in parts]), np.stack([p[name][1] for p in parts]))
            om._rows_equal(merged, whole[name], "%s merged (%s)" % (what, name))
