"""The option matrix of tests/test_option_matrix.py and scripts/fuzz_parity.py: a fixed, seeded table of cases that cross
filtered top-k, range search and code lookup with every dpq_open_opts field, the references of those calls in plain
numpy over the oracle's per-code distances, and the call sequence one opened handle goes through.  No tests in here.

A case is a plain dict; case_id() spells out every option, so a failure names its own reproduction
(`pytest tests/test_option_matrix.py -k <id>`).  Nothing is random at run time: the table is built at import from
np.random.default_rng(TABLE_SEED) and the hand-written MANDATORY list, the same on every machine.

Ids.  A handle reports base + position (base = global_offset, 0 otherwise); the last node of an even-N DTC index is
reported as N, N being the GLOBAL n_codes_total (global_n_codes of a part, num_codes of a prefix, n otherwise).

Choices the issue leaves open, and why:
 * top_k < n wherever n > 1, and below the largest shard: only then can one filter allow MORE codes than top_k.  n = 1
   cannot have more eligible codes than top_k, nor a range list strictly between empty and everything; it is the one
   exemption of the non-vacuity test.
 * radius kinds "exactly the 10th distance" and "nextafter of it" take rank min(9, (n - 1) // 2) of the sorted distances:
   the 10th from n = 20 on, as tests/test_range_search.py, and an interior rank below, so that tiny indexes too have a
   list that is neither empty nor everything.  Radii come from the distances of the whole case (every handle of a
   sharded case gets the same radii, as a sharded search would).
 * a call of fewer than six queries cannot hold the six radius kinds: such a case makes ceil(6 / nq) range calls that
   rotate the kinds.
 * no more shards than segments (an empty shard is no subject of this matrix), no duplicate-heavy tree below 63 codes
   (two equal codes of two leave no interior radius).
 * n = 17 001 and 40 000 always open with bootstrap = 1, 70 001 with 0 (automatic), 20 001 with 0 or -1 (the issue's
   list of sizes).
"""
import numpy as np

TABLE_SEED = 20261018
N_DRAWN = 40

AXES = {
    "n": [1, 2, 3, 63, 64, 65, 127, 129, 255, 257, 4095, 4097, 20001, 17001, 40000, 70001],
    "mkd": [(8, 256, 16), (16, 256, 8), (8, 17, 16), (8, 100, 16), (16, 64, 8), (8, 200, 5)],
    "cps": [1, 2, 4, 8, 16, 64],
    "bd": [-1, 0, 1, 2, 5, 37, 300],
    "boot": [-1, 0, 1],
    "flags": [0, 1, 2, 8, 16, 32, 64, 80, 192],
    "smax": [0, 8, -1],
    "cap": [0, 64, 300],
    "nq": [1, 2, 4, 5, 33, 64, 65, 129, 500],
    "k": [1, 10, 100, 300, 1000, 2048],
    "md": [0.35, 3.0, 6.0],
}
OFFSETS = [1_000_000, 1_000_003, 12_345_678]
# placement kinds: (name, shards, prefix parity or None, offset or None, tail?)
PLACEMENTS = [
    ("whole", 1, None, None, None), ("shards", 2, None, None, None), ("shards", 3, None, None, None),
    ("shards", 5, None, None, None), ("prefix", 1, 1, None, None), ("prefix", 1, 0, None, None),
    ("prefix", 2, 1, None, None), ("prefix", 2, 0, None, None),
    ("part", 1, None, 1_000_000, True), ("part", 1, None, 1_000_000, False),
    ("part", 1, None, 1_000_003, True), ("part", 1, None, 1_000_003, False),
    ("part", 1, None, 12_345_678, True), ("part", 1, None, 12_345_678, False),
]
SLACK = 999_983      # a part that is not the tail: global_n_codes = offset + n + SLACK


def make_case(n, mkd=(8, 256, 16), cps=2, bd=0, boot=0, flags=0, smax=0, cap=0, nq=5, k=10, md=3.0, frac=0.5, shards=1,
              num_codes=0, offset=0, global_n=0, seed=1):
    M, K, Ds = mkd
    return dict(n=n, M=M, K=K, Ds=Ds, cps=cps, bd=bd, boot=boot, flags=flags, smax=smax, cap=cap, nq=nq, k=k, md=md,
                frac=frac, shards=shards, num_codes=num_codes, offset=offset, global_n=global_n, seed=seed)


def case_id(c):
    """Every option, in characters `pytest -k` accepts."""
    return ("n%d_M%d_K%d_Ds%d_cps%d_bd%d_boot%d_fl%d_sm%d_cap%d_nq%d_k%d_md%.2f_fr%g_sh%d_nc%d_off%d_gn%d_s%d" % (
        c["n"], c["M"], c["K"], c["Ds"], c["cps"], c["bd"], c["boot"], c["flags"], c["smax"], c["cap"], c["nq"], c["k"],
        c["md"], c["frac"], c["shards"], c["num_codes"], c["offset"], c["global_n"], c["seed"]))


def n_eff(c):
    """Codes the case's handles hold together."""
    return c["num_codes"] or c["n"]


def n_total(c):
    """N of the even-N rule."""
    return c["global_n"] or c["num_codes"] or c["n"]


def _fit(c):
    """Bring a drawn case inside the choices of the module docstring (deterministic)."""
    n = c["n"]
    if n in (17001, 40000):
        c["boot"] = 1
    elif n == 70001 or (n == 20001 and c["boot"] == 1):
        c["boot"] = 0
    if n < 63 and c["md"] < 1.0:
        c["md"] = 3.0
    if c["num_codes"] and n < 3:
        c["num_codes"] = 0
    ne = n_eff(c)
    n_seg = -(-ne // (64 * c["cps"]))
    c["shards"] = max(s for s in (1, 2, 3, 5) if s <= max(1, min(c["shards"], n_seg)))
    # top_k below the largest shard (segments are dealt out by payload bytes: stay well inside an even split)
    limit = ne if c["shards"] == 1 else (ne // c["shards"]) * 3 // 4
    c["k"] = max([v for v in AXES["k"] if v < limit and v <= c["k"]] or [1])
    return c


def draw_case(rng, axes=None, i=None, n=None):
    """One case.  With `axes` (per-axis value cycles) and an index the draw is stratified: every value of every axis comes
    round; without, every axis is drawn independently, and `n` may be any size (scripts/fuzz_parity.py)."""
    def pick(name, values):
        if axes is not None:
            return axes[name][i % len(axes[name])]
        return values[int(rng.integers(len(values)))]
    v = {name: pick(name, values) for name, values in AXES.items()}
    kind, shards, parity, offset, tail = pick("place", PLACEMENTS)
    n = int(v["n"] if n is None else n)
    c = make_case(n, tuple(int(t) for t in v["mkd"]), int(v["cps"]), int(v["bd"]), int(v["boot"]), int(v["flags"]),
                  int(v["smax"]), int(v["cap"]), int(v["nq"]), int(v["k"]), float(v["md"]),
                  frac=float((0.5, 0.05)[int(rng.integers(2))]), shards=shards, seed=int(rng.integers(1, 1 << 20)))
    if kind == "prefix" and n >= 3:
        p = max(2, (2 * n) // 3)
        c["num_codes"] = p if p % 2 == parity else p - 1
    if kind == "part":
        c["offset"] = offset
        c["global_n"] = offset + n + (0 if tail else SLACK)
    return _fit(c)


def _h(n, **kw):
    return _fit(make_case(n, **kw))


MANDATORY = [
    # an unaligned part that is the global tail with even N (1 000 003 + 4097), and one that is not the tail
    _h(4097, cps=2, bd=2, nq=33, k=100, offset=1_000_003, global_n=1_000_003 + 4097, seed=101),
    _h(4095, cps=4, bd=1, flags=1, nq=64, k=10, md=0.35, offset=12_345_678, global_n=12_345_678 + 4095 + SLACK, seed=102),
    # the unaligned part crossed with bootstrap = 1 at n = 40 000 (even N again: 12 345 678 + 40 000)
    _h(40000, boot=1, bd=5, nq=65, k=300, frac=0.05, offset=12_345_678, global_n=12_345_678 + 40000, seed=103),
    # ... and crossed with n in {1, 65}
    _h(1, nq=2, k=1, offset=1_000_003, global_n=1_000_003 + 1, seed=104),
    _h(65, cps=1, bd=-1, nq=4, k=10, offset=1_000_003, global_n=1_000_003 + 65 + SLACK, seed=105),
    _h(65, cps=8, bd=37, flags=2, nq=129, k=10, offset=12_345_678, global_n=12_345_678 + 65, seed=106),
    # chunks_per_segment = 64 crossed with n in {1, 65, 4097}
    _h(1, cps=64, nq=1, k=1, seed=107),
    _h(65, cps=64, bd=1, nq=5, k=10, seed=108),
    _h(4097, cps=64, bd=2, nq=129, k=1000, md=6.0, shards=2, seed=109),
    # chunks_per_segment = 1 with 5 shards at n = 257
    _h(257, cps=1, bd=5, nq=33, k=10, shards=5, seed=110),
    # (16, 64, 8) with a batch_decode = 37 tile
    _h(20001, mkd=(16, 64, 8), cps=1, bd=37, nq=65, k=2048, md=6.0, seed=111),
    # flags 64 and 192 with nq in {1, 4} on a bootstrap = 1 shard: the filtered call takes the filter scan while the
    # strand image exists
    _h(40000, boot=1, flags=64, nq=1, k=100, shards=2, seed=112),
    _h(40000, boot=1, flags=192, nq=4, k=10, frac=0.05, shards=2, seed=113),
    _h(40000, boot=1, flags=64, nq=4, k=300, md=0.35, shards=2, seed=114),
    _h(40000, boot=1, flags=192, nq=1, k=10, shards=2, seed=115),
    # cand_capacity = 64 with a 0.5 % filter
    _h(70001, cap=64, nq=64, k=100, frac=0.005, seed=116),
    _h(20001, cap=64, boot=-1, bd=1, nq=500, k=10, frac=0.005, seed=117),
    # an even prefix crossed with shards
    _h(20001, cps=4, nq=33, k=100, shards=3, num_codes=13334, seed=118),
    # ... and an odd one with two shards
    _h(4095, cps=2, flags=16, nq=5, k=100, shards=2, num_codes=2731, seed=119),
]


def _build_table():
    rng = np.random.default_rng(TABLE_SEED)
    def cycle(values):       # fresh permutations end to end: every value comes round, the axes stay uncorrelated
        return [values[j] for _ in range(-(-N_DRAWN // len(values))) for j in rng.permutation(len(values))]
    axes = {name: cycle(values) for name, values in AXES.items()}
    axes["place"] = cycle(PLACEMENTS)
    return MANDATORY + [draw_case(rng, axes, i) for i in range(N_DRAWN)]


TABLE = _build_table()


# ---- inputs -----------------------------------------------------------------------------------------------------------

def sub_tree(tree, n_scan):
    """The tree of the first n_scan codes (an even prefix answers like an index holding exactly those)."""
    n_deltas = int(sum(bin(int(m)).count("1") for m in tree["masks"][1:n_scan]))
    return dict(root=tree["root"], depths=tree["depths"][:n_scan], masks=tree["masks"][:n_scan], M=tree["M"],
                deltas=tree["deltas"][:n_deltas])


def build_inputs(c):
    """dict(cb, tree, payload, qs, codes): the seeded inputs of a case.  For K below 256 the tree's root and deltas are
    reduced mod K."""
    from deltapq_amd import synth
    M, K, Ds, seed = c["M"], c["K"], c["Ds"], c["seed"]
    cb = synth.make_codebook(M, K, Ds, seed)
    tree = synth.synth_tree(c["n"], M, seed=seed + 1, mean_diffs=c["md"])
    tree["deltas"] = (tree["deltas"].astype(np.int64) % K).astype(np.uint8)
    tree["root"] = (tree["root"].astype(np.int64) % K).astype(np.uint8)
    payload, _ = synth.encode_dtc(tree)
    qs = synth.make_queries(c["nq"], M * Ds, seed + 2)
    return dict(cb=cb, tree=tree, payload=payload, qs=qs, codes=synth.decode_tree_codes(tree))


def oracle_distances(oracle, c, inp):
    """float32 [nq][n_eff]: the oracle's distance of every code the case's handles hold, by local position."""
    from deltapq_amd import synth
    ne = n_eff(c)
    payload = inp["payload"]
    if c["num_codes"] and c["num_codes"] % 2 == 0:
        payload, _ = synth.encode_dtc(sub_tree(inp["tree"], ne))
    out = np.empty((c["nq"], ne), dtype=np.float32)
    for i, q in enumerate(inp["qs"]):
        out[i] = oracle.scan_lut(payload, ne, oracle.build_lut(inp["cb"], q), 1, want_all=True)[2]
    return out


# ---- references ---------------------------------------------------------------------------------------------------------

def reported_ids(pos, base, N_total):
    """Local positions -> reported ids: base + pos, and N_total for the last node of an even-N index."""
    ids = np.asarray(pos, dtype=np.int64) + int(base)
    if N_total % 2 == 0:
        ids[ids == N_total - 1] = N_total
    return ids


def positions_of(ids, base, N_total):
    """The inverse of reported_ids (ids >= 0 only)."""
    pos = np.asarray(ids, dtype=np.int64).copy()
    if N_total % 2 == 0:
        pos[pos == N_total] = N_total - 1
    return pos - int(base)


def eligible(mask, n_codes, base=0, N_total=None, node_lo=None, node_hi=None):
    """(local positions, reported ids) of the codes of nodes [node_lo, node_hi) (global positions; default: all n_codes
    codes from `base` on) whose reported id r has r < len(mask) and mask[r]."""
    N_total = n_codes if N_total is None else N_total
    lo = 0 if node_lo is None else int(node_lo) - base
    hi = n_codes if node_hi is None else int(node_hi) - base
    assert 0 <= lo <= hi <= n_codes
    pos = np.arange(lo, hi, dtype=np.int64)
    rep = reported_ids(pos, base, N_total)
    ok = rep < len(mask)
    ok[ok] = mask[rep[ok]]
    return pos[ok], rep[ok]


def topk_row(all_d, pos, rep, k):
    """One query's row over the eligible codes: by (distance bits, id), cut to k, padded with -1 / +inf."""
    keys = (all_d[pos].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(pos), dtype=np.uint64)
    if len(keys) > k:                                     # (rep ascends with pos: the index orders like the id)
        keys = np.partition(keys, k - 1)[:k]
    sel = (np.sort(keys) & np.uint64(0xffffffff)).astype(np.int64)
    ids = np.full(k, -1, dtype=np.int32)
    d = np.full(k, np.inf, dtype=np.float32)
    ids[:len(sel)] = rep[sel]
    d[:len(sel)] = all_d[pos[sel]]
    return ids, d


def expected_topk(all_d, mask, k, base=0, N_total=None, node_lo=None, node_hi=None):
    """The filtered answer of one query on the handle that holds nodes [node_lo, node_hi): all_d[p] is the distance of
    local position p, `mask` a bool array over reported ids."""
    pos, rep = eligible(mask, len(all_d), base, N_total, node_lo, node_hi)
    return topk_row(all_d, pos, rep, k)


def expected_range(all_d, r, base=0, N_total=None, node_lo=None, node_hi=None):
    """(ids int32, dists) of one query's range list on that handle: d < r strictly, by (distance bits, id); r = +inf:
    every code of the handle, those at +inf included (include/deltapq_amd.h, range search)."""
    N_total = len(all_d) if N_total is None else N_total
    lo = 0 if node_lo is None else int(node_lo) - base
    hi = len(all_d) if node_hi is None else int(node_hi) - base
    pos = lo + (np.arange(hi - lo) if np.isposinf(r) else np.flatnonzero(all_d[lo:hi] < np.float32(r)))
    pos = pos[np.lexsort((pos, all_d[pos].view(np.uint32)))]
    return reported_ids(pos, base, N_total).astype(np.int32), all_d[pos]


RADIUS_KINDS = ("zero", "below the minimum", "exactly the 10th distance", "nextafter of it", "median", "+inf")


def radius_menu(all_d, i):
    """Radius kind i % 6 for one query's distances (see the module docstring for the rank of "the 10th")."""
    s = np.sort(all_d)
    tenth = s[min(9, (len(s) - 1) // 2)]
    kind = i % 6
    if kind == 0:
        return np.float32(0.0)
    if kind == 1:
        return np.float32(s[0] * np.float32(0.5)) if s[0] > 0 else np.float32(0.0)
    if kind == 2:
        return tenth
    if kind == 3:
        return np.nextafter(tenth, np.float32(np.inf))
    if kind == 4:
        return s[len(s) // 2]
    return np.float32(np.inf)


def radii_calls(c, alld):
    """One float32 [nq] array of radii per range call of the case."""
    nq = c["nq"]
    calls = 1 if nq >= 6 else -(-6 // nq)
    return [np.array([radius_menu(alld[i], i + j * nq) for i in range(nq)], dtype=np.float32) for j in range(calls)]


def make_masks(c):
    """[(name, bool mask over reported ids)]: all ones with n_bits beyond the id range; random at the case's fraction with
    n_bits short of it (no multiple of 32); a few ids (under top_k) with n_bits exact -- bit N set and bit N - 1 clear
    where the case holds the even-N tail (top_k = 1 leaves room for no id: then bit N - 1 alone, which governs nothing)."""
    rng = np.random.default_rng(c["seed"] + 3)
    base, ne, N = c["offset"], n_eff(c), n_total(c)
    rep = reported_ids(np.arange(ne), base, N)
    tail_even = N % 2 == 0 and base + ne == N
    id_end = int(rep.max()) + 1
    ones = np.ones(id_end + 37, dtype=bool)
    short = id_end - max(1, ne // 5)
    if short % 32 == 0 and short > 0:
        short -= 1
    rnd = np.ones(short, dtype=bool)                       # (bits below the base govern nothing on these handles)
    if short > base:
        rnd[base:] = rng.random(short - base) < c["frac"]
    few = np.zeros(id_end, dtype=bool)
    pool = rep[:-1] if tail_even else rep
    room = c["k"] - 1 - (1 if tail_even else 0)
    cnt = max(0, min(room, 37, len(pool)))
    if cnt:
        few[rng.choice(pool, cnt, replace=False)] = True
    if tail_even:
        few[N if c["k"] >= 2 else N - 1] = True
    return [("ones", ones), ("random", rnd), ("few", few)]


def call_k(c):
    """top_k of every call of the case: the largest the library takes (top_k <= n_codes_total)."""
    return min(c["k"], n_total(c))


def handle_reference(c, alld, masks, radii, node_lo, node_hi):
    """What the handle over nodes [node_lo, node_hi) must answer: dict(filtered={name: (n_allowed, [(ids, d)] per
    query)}, ranges=[[(ids, d)] per query] per range call)."""
    base, N, k = c["offset"], n_total(c), call_k(c)
    filtered = {}
    for name, mask in masks:
        pos, rep = eligible(mask, alld.shape[1], base, N, node_lo, node_hi)
        filtered[name] = (len(pos), [topk_row(alld[q], pos, rep, k) for q in range(c["nq"])])
    ranges = [[expected_range(alld[q], r[q], base, N, node_lo, node_hi) for q in range(c["nq"])] for r in radii]
    return dict(filtered=filtered, ranges=ranges)


def handle_bounds(c, inp):
    """[(node_lo, node_hi)] in global positions of every handle of the case, from the host transcoder (no GPU)."""
    from deltapq_amd import api
    if c["shards"] == 1:
        return [(c["offset"], c["offset"] + n_eff(c))]
    out = []
    for rank in range(c["shards"]):
        info = api.HostSoA(inp["payload"], c["n"], c["M"], shard_rank=rank, shard_count=c["shards"],
                           chunks_per_segment=c["cps"], num_codes=c["num_codes"]).info
        out.append((c["offset"] + info["node_lo"], c["offset"] + info["node_hi"]))
    return out


# ---- the call sequence ------------------------------------------------------------------------------------------------------

def open_kwargs(c, rank=0):
    return dict(chunks_per_segment=c["cps"], cand_capacity=c["cap"], shard_rank=rank, shard_count=c["shards"],
                num_codes=c["num_codes"], bootstrap=c["boot"], global_offset=c["offset"], global_n_codes=c["global_n"],
                batch_decode=c["bd"], flags=c["flags"], stream_max_queries=c["smax"])


def _rows_equal(got, want, what):
    gi, gd = got
    assert len(gi) == len(gd) == len(want), what
    for q, (wi, wd) in enumerate(want):
        assert np.array_equal(gd[q].view(np.uint32), wd.view(np.uint32)), "%s query %d: distances differ\n got %s\n want %s" % (
            what, q, gd[q][:8], wd[:8])
        assert np.array_equal(gi[q], wi), "%s query %d: ids differ\n got %s\n want %s" % (what, q, gi[q][:8], wi[:8])


def _range_equal(got, want, what):
    lims, ids, dists = got
    assert len(lims) == len(want) + 1 and lims[0] == 0, what
    for q, (wi, wd) in enumerate(want):
        gi, gd = ids[lims[q]:lims[q + 1]], dists[lims[q]:lims[q + 1]]
        assert len(gi) == len(wi), "%s query %d: %d results, expected %d" % (what, q, len(gi), len(wi))
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), "%s query %d: distances differ" % (what, q)
        assert np.array_equal(gi, wi), "%s query %d: ids differ" % (what, q)


def check_handle(api, idx, c, inp, alld, masks, radii, what):
    """The five steps on one open handle, every query of every call against the reference.  Returns what the handle
    answered (for the merge of a sharded case): dict(filtered={name: (ids, d)}, ranges=[(lims, ids, d)])."""
    from oracle.dtc_oracle import tie_aware_equal
    info = idx.info()
    lo, hi = info["node_lo"], info["node_hi"]
    base, N, k, qs = c["offset"], n_total(c), call_k(c), inp["qs"]
    assert info["n_codes_total"] == N and base <= lo <= hi <= base + n_eff(c), "%s: nodes [%d, %d)" % (what, lo, hi)
    ref = handle_reference(c, alld, masks, radii, lo, hi)
    # 1. unfiltered, tie-aware against the oracle's distances of this handle's nodes
    first = idx.query_batch(qs, k)
    cnt = min(k, hi - lo)
    for q, (wi, wd) in enumerate(ref["filtered"]["ones"][1]):
        gi, gd = first[0][q], first[1][q]
        assert np.all(gi[cnt:] == -1) and np.all(np.isposinf(gd[cnt:])), "%s unfiltered query %d: padding" % (what, q)
        assert np.all(gi[:cnt] >= 0), "%s unfiltered query %d: a padded row among %d codes" % (what, q, hi - lo)
        assert np.array_equal(reported_ids(positions_of(gi[:cnt], base, N), base, N), gi[:cnt]) and \
            np.all((gi[:cnt] >= lo) & (gi[:cnt] <= max(hi - 1, N if N % 2 == 0 and hi == N else 0))), \
            "%s unfiltered query %d: an id this handle cannot report in %s" % (what, q, gi[:8])
        ok, msg = tie_aware_equal(positions_of(gi[:cnt], base, N), gd[:cnt], positions_of(wi[:cnt], base, N), wd[:cnt], alld[q])
        assert ok, "%s unfiltered query %d: %s\n got %s %s\n want %s %s" % (what, q, msg, gi[:8], gd[:4], wi[:8], wd[:4])
    # 2. filtered: three masks over reported ids
    out = dict(filtered={}, ranges=[])
    for name, mask in masks:
        with api.IdFilter.from_mask(idx, mask) as f:
            assert f.n_allowed == ref["filtered"][name][0], "%s mask %s: n_allowed %d, expected %d" % (
                what, name, f.n_allowed, ref["filtered"][name][0])
            got = idx.query_batch_filtered(qs, k, f)
        _rows_equal(got, ref["filtered"][name][1], "%s filtered (%s, n_bits=%d)" % (what, name, len(mask)))
        if name == "ones":
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1].view(np.uint32), first[1].view(np.uint32)), \
                "%s: the all-ones filter differs from the unfiltered call" % what
        out["filtered"][name] = got
    # 3. range search
    for j, r in enumerate(radii):
        got = idx.range_search(qs, r)
        _range_equal(got, ref["ranges"][j], "%s range call %d" % (what, j))
        out["ranges"].append(got)
    # 4. code lookup of the filtered rows, padding included
    for name in ("random", "few"):
        ids = out["filtered"][name][0].reshape(-1)
        want = np.zeros((len(ids), c["M"]), dtype=np.uint8)
        real = ids >= 0
        want[real] = inp["codes"][positions_of(ids[real], base, N)]
        assert np.array_equal(idx.get_codes(ids), want), "%s get_codes of the filtered rows (%s)" % (what, name)
    # 5. the unfiltered call again: the same bits
    again = idx.query_batch(qs, k)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1].view(np.uint32), first[1].view(np.uint32)), \
        "%s: the unfiltered answer changed after filtered, range and lookup calls" % what
    return out


def run_case(api, oracle, c, inp=None, alld=None):
    """Every handle of the case through check_handle; a sharded case's merged answers against the whole-index
    expectation from the oracle."""
    from deltapq_amd.dist import merge_range_host
    what = case_id(c)
    inp = build_inputs(c) if inp is None else inp
    alld = oracle_distances(oracle, c, inp) if alld is None else alld
    masks, radii = make_masks(c), radii_calls(c, alld)
    parts = []
    for rank in range(c["shards"]):
        with api.DeltaPQIndex.open_memory(inp["payload"], c["n"], c["M"], c["K"], **open_kwargs(c, rank)) as idx:
            idx.set_codebook(inp["cb"])
            parts.append(check_handle(api, idx, c, inp, alld, masks, radii,
                                      what if c["shards"] == 1 else "%s rank %d" % (what, rank)))
    if c["shards"] > 1:
        whole = handle_reference(c, alld, masks, radii, None, None)
        for name, _ in masks:
            merged = api.merge_topk_host(np.stack([p["filtered"][name][0] for p in parts]),
                                         np.stack([p["filtered"][name][1] for p in parts]))
            _rows_equal(merged, whole["filtered"][name][1], "%s merged filtered (%s)" % (what, name))
        for j in range(len(radii)):
            _range_equal(merge_range_host([p["ranges"][j] for p in parts]), whole["ranges"][j],
                         "%s merged range call %d" % (what, j))
