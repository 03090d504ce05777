"""Candidate search and inner-product search crossed with the option matrix of tests/_option_matrix.py, and handles whose
ids lie at the top of the int32 range: the candidate lists, the references and the call sequences of
tests/test_matrix_candidates_ip.py.  No tests in here, and nothing but numpy.

The per-code distances `alld` [nq][n] of a case (om.oracle_distances) serve every L2 form; the per-code gaps `g` come from
T.ip_tables and T.distances_dtc.  A "geometry" is (base, n, N): the first global position the case's handles hold
together, how many codes they hold, and the N of the even-N rule.  Every comparison is strict: ids and float bits.

Choices the issue leaves open, and why:
 * the wide list's window starts at rng.integers(n) and is permuted with rng.permutation; "every fifth entry again" are
   the entries [::5] of the list as it stands after the first -1 went in.
 * the refused call replaces entry [nq // 2][0], a real id in every case (the first entry of a row is never padding).
 * the filters of the top-of-range handles: the range [lo + n // 2, past the handle's last reported id) where the handle
   holds the tail (so it crosses the tail id) and [lo + n // 4, lo + n // 4 + n // 2) elsewhere; 37 ids drawn without
   replacement from the handle's reported ids (all of them below 37 codes), plus the tail id where the handle holds it.
"""
import numpy as np

import _candidates_restatement as C
import _option_matrix as om
import _tables_restatement as T

ERR_ARG = -1
TOP = 2 ** 31 - 2            # the largest global_offset + n_codes, and the largest global_n_codes, a handle opens with
WINDOW = 4000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def geometry(c):
    return c["offset"], om.n_eff(c), om.n_total(c)


def holds_even_tail(geo):
    base, n, N = geo
    return N % 2 == 0 and base + n == N


def id_rules(lo, hi, N):
    """The keyword arguments of C.classify / C.search_row for the handle over nodes [lo, hi)."""
    return dict(id_base=lo, n_local=hi - lo, n_total=N, even_rule=True)


# ---- the lists -----------------------------------------------------------------------------------------------------------

def _padded(rows, width):
    out = np.full((len(rows), width), -1, dtype=np.int32)
    for q, r in enumerate(rows):
        out[q, :len(r)] = r
    return out


def make_lists(c, geo=None):
    """dict(wide int32 [nq][W], few int32 [nq][k + 2]) of a case, the same for every handle of it.  `geo`: the geometry
    where it is not the case's own (two adjacent parts share the lists of the pair)."""
    rng = np.random.default_rng(c["seed"] + 5)
    base, n, N = geo = geometry(c) if geo is None else geo
    nq, k = c["nq"], om.call_k(c)
    rep = om.reported_ids(np.arange(n), base, N)
    w = min(n, WINDOW)
    extra = []
    if base > 0:
        extra += [base - 1, 0]
    if base + n != N:
        extra += [base + n, N if N % 2 == 0 else N - 1]
    if holds_even_tail(geo):
        extra += [N]
    wide = []
    for q in range(nq):
        win = rep[(int(rng.integers(n)) + np.arange(w)) % n]
        win = win[rng.permutation(w)]
        row = np.concatenate([win[:1], [-1], win[1:]])
        wide.append(np.concatenate([row, row[::5], [-1], extra]).astype(np.int64))
    few = [rng.choice(rep, q % min(k, 10), replace=False) for q in range(nq)]
    return dict(wide=_padded(wide, max(len(r) for r in wide)), few=_padded(few, k + 2))


def bad_id(geo):
    """An id that names no node of the index: N - 1 where the case holds the even-N tail, else N (odd) or N + 1 (even)."""
    N = geo[2]
    if holds_even_tail(geo):
        return N - 1
    return N if N % 2 else N + 1


def list_facts(c, bounds, lists, geo=None):
    """What test_no_list_is_vacuous asserts, on the references alone: dict(none, wide_distinct, few_distinct, skipped,
    tail_listed) over the handles `bounds` [(lo, hi)]."""
    geo = geometry(c) if geo is None else geo
    N = geo[2]
    none, skipped, tail_listed, wide_distinct, few_distinct = 0, False, False, 0, 0
    for lo, hi in bounds:
        r = id_rules(lo, hi, N)
        for name in ("wide", "few"):
            cls, local = C.classify(lists[name], **r)
            none += int((cls == C.NONE).sum())
            skipped |= bool(((cls == C.SKIP) & (lists[name] >= 0)).any())
            distinct = max(len(np.unique(row[row >= 0])) for row in local)
            if name == "wide":
                wide_distinct = max(wide_distinct, distinct)
                if holds_even_tail(geo) and hi == N:
                    tail_listed |= bool(((lists[name] == N) & (cls == C.LOCAL)).any())
            else:
                few_distinct = max(few_distinct, distinct)
    return dict(none=none, wide_distinct=wide_distinct, few_distinct=few_distinct, skipped=skipped, tail_listed=tail_listed)


# ---- inner product: the reference --------------------------------------------------------------------------------------------

def table_is_exact(table):
    """The condition of ne.table_units (include/deltapq_amd.h "exact tables") on one fp32 table [M][K], in numpy: the
    finite non-zero entries are whole multiples of 2^g, g the lowest set bit among them, and the per-row maxima add up to
    less than 2^53 of these units."""
    t = np.asarray(table, dtype=np.float32)
    v = t[np.isfinite(t) & (t != 0)].astype(np.float64)
    if v.size == 0:
        return True
    mant, exp = np.frexp(v)
    m24 = np.ldexp(mant, 24).astype(np.int64)                 # an fp32 significand is a whole number of 24 bits
    assert np.all(np.ldexp(m24.astype(np.float64), exp - 24) == v)
    g = int((exp - 24 + np.log2((m24 & -m24).astype(np.float64)).astype(np.int64)).min())
    total = 0
    for row in t:
        fin = row[np.isfinite(row)]
        if fin.size:
            total += int(np.ldexp(np.float64(fin.max()), -g))   # a power-of-two scaling: exact, and a whole number
    return total < 2 ** 53


def ip_reference(c, inp):
    """dict(e [nq][M][K], B [nq], g [nq][n], exact bool [nq]) by the rules of the header."""
    n = om.n_eff(c)
    _, _, e, B = T.ip_tables(inp["cb"], inp["qs"])
    codes = inp["codes"][:n]
    g = np.empty((c["nq"], n), dtype=np.float32)
    for q in range(c["nq"]):                                  # one query at a time: [nq][n][M] would not fit
        g[q] = T.distances_dtc(e[q], codes)
    return dict(e=e, B=B, g=g, exact=np.array([table_is_exact(t) for t in e]))


def ip_rows(g, B, pos, rep, k):
    """(ids [nq][k], gaps, scores) over the eligible codes (pos, rep)."""
    rows = [om.topk_row(gq, pos, rep, k) for gq in g]
    ids, gaps = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    return ids, gaps, T.ip_scores(B, gaps, ids)


def check_ip(got, want, B, what):
    """check() of tests/test_ip_search.py: ids, gap bits, score bits, bias bits, the padding."""
    ids, scores, gaps, bias = got
    assert np.array_equal(bits(bias), bits(B)), what + ": bias"
    assert np.array_equal(bits(gaps), bits(want[1])), what + ": gaps"
    assert np.array_equal(ids, want[0]), what + ": ids"
    assert np.array_equal(bits(scores), bits(want[2])), what + ": scores"
    real = ids >= 0
    assert np.all(np.isposinf(gaps[~real])) and np.all(np.isneginf(scores[~real])), what + ": padding"
    s = np.where(real, scores, -np.inf)
    assert np.all(s[:, :-1] >= s[:, 1:]), what + ": scores do not descend"


# ---- the call sequences --------------------------------------------------------------------------------------------------------

def _status(api, call):
    try:
        call()
    except api.DpqError as e:
        return e.status
    return 0


def candidate_calls(api, idx, c, inp, alld, lists, what, geo=None, before_codebook=False):
    """The candidate calls of one handle, opened WITHOUT a codebook (the function sets it).  alld [nq][n] holds the
    distances of the geometry's codes by position.  Returns dict(first=query_batch's answer, wide=the wide answer at k)."""
    import torch
    base, n, N = geo = geometry(c) if geo is None else geo
    info = idx.info()
    lo, hi = info["node_lo"], info["node_hi"]
    assert info["n_codes_total"] == N and base <= lo < hi <= base + n, "%s: nodes [%d, %d)" % (what, lo, hi)
    k, qs, nq = om.call_k(c), inp["qs"], c["nq"]
    wide, few = lists["wide"], lists["few"]
    n_cand = wide.shape[1]
    d = alld[:, lo - base:hi - base]
    r = id_rules(lo, hi, N)
    tabs = T.l2_tables(inp["cb"], qs)

    def want(cand, kk):
        return [C.search_row(d[q], cand[q], kk, **r) for q in range(nq)]

    want_k = want(wide, k)
    if before_codebook:
        om._rows_equal(idx.candidate_search_tables(tabs, wide, k), want_k, what + " tables form, no codebook")
    idx.set_codebook(inp["cb"])
    first = idx.query_batch(qs, k)
    # the wide list
    for kk in sorted({1, k} | ({n_cand} if n_cand <= 2048 else set())):
        om._rows_equal(idx.candidate_search(qs, wide, kk), want(wide, kk), "%s wide top-%d of %d" % (what, kk, n_cand))
    got_k = idx.candidate_search(qs, wide, k)
    # fewer valid ids than top_k; query 0 has none
    got = idx.candidate_search(qs, few, k)
    om._rows_equal(got, want(few, k), what + " few")
    assert np.all(got[0][0] == -1) and np.all(np.isposinf(got[1][0])), what + " few: query 0 is not all padding"
    # the distances, in place
    dist = idx.candidate_distances(qs, wide)
    want_d = np.stack([C.candidate_distances(d[q], wide[q], **r) for q in range(nq)])
    cls, local = C.classify(wide, **r)
    assert np.array_equal(np.isnan(dist), cls != C.LOCAL), what + " distances: NaN exactly where the entry is not local"
    assert np.array_equal(bits(dist), bits(want_d)), what + " distances"
    # the tables form
    by_t = idx.candidate_search_tables(tabs, wide, k)
    om._rows_equal(by_t, want_k, what + " tables form")
    assert same(by_t, got_k), what + ": the tables form differs from the query form"
    # the handle's own answer as the list
    assert same(idx.candidate_search(qs, first[0], k), first), what + ": own ids as candidates differ from query_batch"
    # the device forms
    t_q, t_w = torch.from_numpy(qs).cuda(), torch.from_numpy(wide).cuda()
    ti, td = idx.candidate_search_torch(t_q, t_w, k)
    om._rows_equal((ti.cpu().numpy(), td.cpu().numpy()), want_k, what + " wide, device form")
    assert np.array_equal(bits(idx.candidate_distances_torch(t_q, t_w).cpu().numpy()), bits(want_d)), \
        what + " distances, device form"
    # an id that names no node: refused by both forms, and the next call answers as before
    bad = wide.copy()
    bad[nq // 2, 0] = bad_id(geo)
    assert np.all(wide[:, 0] >= 0)
    t_b = torch.from_numpy(bad).cuda()
    assert _status(api, lambda: idx.candidate_search(qs, bad, k)) == ERR_ARG, "%s: id %d, host form" % (what, bad_id(geo))
    assert _status(api, lambda: idx.candidate_search_torch(t_q, t_b, k)) == ERR_ARG, "%s: id %d, device form" % (what, bad_id(geo))
    assert _status(api, lambda: idx.candidate_distances(qs, bad)) == ERR_ARG, "%s: id %d, distances" % (what, bad_id(geo))
    assert same(idx.candidate_search(qs, wide, k), got_k), what + ": the wide answer changed after refused calls"
    om._rows_equal(got_k, want_k, what + " wide")
    again = idx.query_batch(qs, k)
    assert same(again, first), what + ": query_batch changed after the candidate calls"
    return dict(first=first, wide=got_k)


def run_candidates(api, c, inp, alld, lists):
    """Every handle of a case of om.TABLE through candidate_calls; a sharded case's merged wide answer against the
    whole-case expectation."""
    what = om.case_id(c)
    base, n, N = geometry(c)
    parts = []
    for rank in range(c["shards"]):
        with api.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c, rank)) as idx:
            parts.append(candidate_calls(api, idx, c, inp, alld, lists, what if c["shards"] == 1 else "%s rank %d" % (what, rank),
                                         before_codebook=rank == 0))
    if c["shards"] > 1:
        k = om.call_k(c)
        merged = api.merge_topk_host(np.stack([p["wide"][0] for p in parts]), np.stack([p["wide"][1] for p in parts]))
        whole = [C.search_row(alld[q], lists["wide"][q], k, **id_rules(base, base + n, N)) for q in range(c["nq"])]
        om._rows_equal(merged, whole, what + " merged wide")


def ip_calls(api, idx, c, inp, ref, mask, what, geo=None):
    """The inner-product calls of one handle (codebook set).  `mask`: a bool mask over reported ids, or None.  Returns
    (ids, scores, gaps, bias) of the unfiltered call."""
    import torch
    base, n, N = geometry(c) if geo is None else geo
    info = idx.info()
    lo, hi = info["node_lo"], info["node_hi"]
    k, qs, nq = om.call_k(c), inp["qs"], c["nq"]
    assert ref["exact"].all(), what + ": a table of this case is not exact; its gaps are not defined to the bit"
    pos = np.arange(lo - base, hi - base)
    want = ip_rows(ref["g"], ref["B"], pos, om.reported_ids(pos, base, N), k)
    got = idx.query_batch_ip(qs, k)
    check_ip(got, want, ref["B"], what + " query_batch_ip")
    if mask is not None:
        with api.IdFilter.from_mask(idx, mask) as f:
            fil = idx.query_batch_ip(qs, k, id_filter=f)
        check_ip(fil, ip_rows(ref["g"], ref["B"], *om.eligible(mask, n, base, N, lo, hi), k), ref["B"],
                 what + " query_batch_ip, filtered")
    gaps = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    bias = torch.empty((nq,), dtype=torch.float32, device="cuda")
    ids, scores = idx.query_batch_ip_torch(torch.from_numpy(qs).cuda(), k, out_gaps=gaps, out_bias=bias)
    check_ip((ids.cpu().numpy(), scores.cpu().numpy(), gaps.cpu().numpy(), bias.cpu().numpy()), want, ref["B"],
             what + " query_batch_ip, device form")
    return got


def run_ip(api, c, inp, ref, mask):
    what = om.case_id(c)
    base, n, N = geometry(c)
    parts = []
    for rank in range(c["shards"]):
        with api.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **om.open_kwargs(c, rank)) as idx:
            idx.set_codebook(inp["cb"])
            parts.append(ip_calls(api, idx, c, inp, ref, mask, what if c["shards"] == 1 else "%s rank %d" % (what, rank)))
    if c["shards"] > 1:
        for p in parts[1:]:
            assert np.array_equal(bits(p[3]), bits(parts[0][3])), what + ": the bias depends on the shard"
        ids, gaps = api.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[2] for p in parts]))
        pos = np.arange(n)
        want = ip_rows(ref["g"], ref["B"], pos, om.reported_ids(pos, base, N), om.call_k(c))
        check_ip((ids, api.ip_scores(parts[0][3], gaps, ids), gaps, parts[0][3]), want, ref["B"], what + " merged")


# ---- handles at the top of the id range ------------------------------------------------------------------------------------------

def _top(n, tail=TOP, **kw):
    """A part whose last node is global position tail - 1."""
    return om.make_case(n, offset=tail - n, global_n=tail, **kw)


def _mid(n, offset, **kw):
    return om.make_case(n, offset=offset, global_n=offset + n + om.SLACK, **kw)


TOP_CASES = [
    _top(65, cps=1, nq=4, k=10, seed=201),
    _mid(4097, 2_000_000_003, cps=2, bd=2, nq=33, k=100, seed=202),
    _top(4097, tail=TOP - 1, bd=1, nq=129, k=1000, seed=203),
    _mid(4097, 2 ** 30 - 2000, nq=65, k=100, seed=204),
    _top(40000, boot=1, flags=64, nq=1, k=100, seed=205),
    _top(40000, boot=1, flags=192, nq=4, k=10, seed=206),
    _top(17001, boot=1, nq=65, k=300, seed=207),
    _top(20001, mkd=(16, 64, 8), cps=1, bd=37, nq=65, k=1000, seed=208),
]
# two adjacent parts of two payloads; the second is the even-N tail at 2^31 - 2.  One seed: one codebook, one set of queries.
TOP_PAIR = [om.make_case(4095, nq=33, k=100, offset=TOP - 4097 - 4095, global_n=TOP, seed=209),
            om.make_case(4097, nq=33, k=100, offset=TOP - 4097, global_n=TOP, seed=209)]
PAIR_GEO = (TOP - 4097 - 4095, 4095 + 4097, TOP)


def top_filters(c, lo, hi, geo=None):
    """((range_lo, range_hi), listed ids int32) for the handle over nodes [lo, hi) (see the module docstring)."""
    geo = geometry(c) if geo is None else geo
    N = geo[2]
    n = hi - lo
    rep = om.reported_ids(np.arange(n), lo, N)
    tail = holds_even_tail(geo) and hi == N
    rng = np.random.default_rng(c["seed"] + 7 + lo % 1000)
    listed = rng.choice(rep[:-1] if tail else rep, min(37, n - (1 if tail else 0)), replace=False)
    if tail:
        listed = np.concatenate([listed, [N]])
    rg = (lo + n // 2, int(rep.max()) + 1) if hi == N else (lo + n // 4, lo + n // 4 + n // 2)
    return rg, listed.astype(np.int32)


def top_calls(api, idx, c, inp, alld, ref, lists, what, geo=None, before_codebook=True):
    """The call sequence of one handle near the top of the id range (opened without a codebook).  alld and ref["g"] hold
    the geometry's codes by position.  Returns dict(first, wide)."""
    base, n, N = geo = geometry(c) if geo is None else geo
    out = candidate_calls(api, idx, c, inp, alld, lists, what, geo, before_codebook)     # sets the codebook
    info = idx.info()
    lo, hi = info["node_lo"], info["node_hi"]
    k, qs, nq = om.call_k(c), inp["qs"], c["nq"]
    pos = np.arange(lo - base, hi - base)
    rep = om.reported_ids(pos, base, N)
    codes = inp["codes"]                                       # this handle's payload: position p - (lo - base)
    om._rows_equal(out["first"], [om.topk_row(alld[q], pos, rep, k) for q in range(nq)], what + " query_batch")
    (r_lo, r_hi), listed = top_filters(c, lo, hi, geo)
    in_range = (rep >= r_lo) & (rep < r_hi)
    in_list = np.isin(rep, listed)
    assert in_range.any() and not in_range.all() and in_list.sum() == len(listed)
    for name, ok, make in (("range [%d, %d)" % (r_lo, r_hi), in_range, lambda: api.IdFilter.from_range(idx, r_lo, r_hi)),
                           ("%d listed ids" % len(listed), in_list, lambda: api.IdFilter.from_ids(idx, listed))):
        with make() as f:
            assert f.n_allowed == ok.sum(), "%s %s: n_allowed %d, expected %d" % (what, name, f.n_allowed, ok.sum())
            got = idx.query_batch_filtered(qs, k, f)
        om._rows_equal(got, [om.topk_row(alld[q], pos[ok], rep[ok], k) for q in range(nq)], "%s filtered (%s)" % (what, name))
        ids = got[0].reshape(-1)
        want = np.zeros((len(ids), c["M"]), dtype=np.uint8)
        real = ids >= 0
        want[real] = codes[om.positions_of(ids[real], lo, N)]
        assert np.array_equal(idx.get_codes(ids), want), "%s get_codes of the filtered rows (%s)" % (what, name)
    for j, radii in enumerate(om.radii_calls(c, alld)):
        om._range_equal(idx.range_search(qs, radii), [om.expected_range(alld[q], radii[q], base, N, lo, hi) for q in range(nq)],
                        "%s range call %d" % (what, j))
    ip_calls(api, idx, c, inp, ref, None, what, geo)
    assert same(idx.query_batch(qs, k), out["first"]), what + ": query_batch changed after the whole sequence"
    return out
