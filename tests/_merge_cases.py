"""The hand-built partial top-k lists of tests/test_merge.py: a fixed, seeded table of cases for dpq_merge_topk_host,
dpq_merge_topk_device and dpq_merge_topk_device_packed, the reference of the merge in plain numpy, and two restatements
of the merge kernel's rank rule (the strict one it had, the stable one it has).  No tests in here.

A case is a plain dict (n_lists, top_k, nq, fill, seed); case_id() spells all five out, so a failure names its own
reproduction (`pytest tests/test_merge.py -k <id>`).  Nothing is random at run time: TABLE is built at import from the
lists below, and build_lists() draws a case's rows from np.random.default_rng over the case's own fields.

What a list is.  ids int32 / dists float32 [n_lists][nq][top_k]; every list ascending by (distance bit pattern as
uint32, id) with its padding rows (id < 0) last -- the contract of the device calls.

The reference (reference()): per query every row with id >= 0 of all lists, np.lexsort by (bits, id), the first top_k,
padded with (-1, +inf).  Repeated keys are kept as often as they occur.

Fill kinds (FILLS), and the choices the issue leaves open:
 * full         every list holds top_k valid rows, distinct keys.
 * ragged       every list holds 0 .. top_k valid rows; per query one list is empty and one is full (n_lists >= 2).
 * short        fewer than top_k valid rows in total, so the output ends in padding (top_k >= 2: at least one row).
 * all_empty    no valid row; the padding rows are the plain (-1, +inf).
 * ties         distances from TIE_POOL (three bit patterns), ids disjoint.  Query 0 draws ONE pattern for all its rows
                (every row ties, the order is the ids'), the other queries draw from all three; every list is full.
                "Equal bits in two different lists on both sides of rank top_k" is read as: the bits of merged row
                top_k - 1 are also the bits of merged row top_k (the first row cut), and a row of those bits that is
                kept and one that is cut come from different lists.  ties_straddle() checks it from the data.
 * interleaved  list l holds keys l, l + n_lists, l + 2 n_lists, ... of one global order: every search lands mid-list.
 * one_wins_first / one_wins_last
                list 0 / the last list lies wholly below all others and is full: searches in it return top_k, searches
                of its keys in the others return 0.
 * edges_of_value
                top_k // 2 finite rows, a third of them distance 0.0, and top_k // 2 + 2 valid rows of distance +inf (so
                the +inf rows reach the output ahead of the padding and are cut by id; with one list top_k // 4 + 1 of
                them, which leaves the list padding rows and cuts nothing), dealt over the lists; ids
                2^31 - 1 and 0 among them (2^31 - 1 on a 0.0 row when there is one); padding rows carry ids -1, -2,
                -2^31 or a random negative one and distances 0.0, -1.0, a NaN, +inf or a random one.
 * dups         keys that occur more than once, by query: q % 3 == 0 the same rows in lists 0 and 1, q % 3 == 1 the
                same rows in ALL lists, q % 3 == 2 a key twice inside list 0 and once more in the last list; around
                them distinct rows.  The repeated keys are the smallest of the query, so they fall inside top_k
                (top_k >= 2, n_lists >= 2: with top_k = 1 two copies of the best key answer like one).
"""
import functools

import numpy as np

SHAPES = [      # (n_lists, top_k, nq): each the smallest that reaches its edge
    (1, 1, 1),          # smallest
    (1, 2048, 3),       # one long list
    (2, 1, 5),          # k = 1
    (3, 7, 65),         # small odd k
    (2, 511, 2), (2, 512, 2), (2, 513, 2),      # around the 512 threads of the block
    (5, 257, 4),        # odd k, several lists
    (8, 100, 33),       # the sharded path's own shape
    (8, 2048, 2), (16, 1024, 2),                # exactly 16384 keys = 128 KB of LDS
    (7, 2340, 1),       # 16380 keys, not a power of two
    (16384, 1, 2),      # most lists, k = 1
    (4, 300, 1000),     # many blocks
]
LDS_EDGE = [(8, 2048, 2), (16, 1024, 2)]

FILLS = {       # fill kind -> the shapes it is crossed with
    "full": SHAPES,
    "ragged": [(3, 7, 65), (2, 512, 2), (5, 257, 4), (8, 100, 33), (16384, 1, 2), (4, 300, 1000)] + LDS_EDGE,
    "short": [(1, 2048, 3), (3, 7, 65), (2, 513, 2), (8, 100, 33), (7, 2340, 1)],
    "all_empty": [(1, 1, 1), (2, 1, 5), (3, 7, 65), (8, 2048, 2), (16384, 1, 2)],
    "ties": [(2, 1, 5), (3, 7, 65), (2, 511, 2), (2, 512, 2), (2, 513, 2), (8, 100, 33), (16384, 1, 2),
             (4, 300, 1000)] + LDS_EDGE,
    "interleaved": [(2, 1, 5), (3, 7, 65), (2, 513, 2), (5, 257, 4), (7, 2340, 1), (16, 1024, 2)],
    "one_wins_first": [(2, 1, 5), (3, 7, 65), (2, 512, 2), (5, 257, 4), (8, 100, 33), (16, 1024, 2)],
    "one_wins_last": [(2, 1, 5), (3, 7, 65), (2, 512, 2), (5, 257, 4), (8, 100, 33), (16, 1024, 2)],
    "edges_of_value": [(1, 1, 1), (1, 2048, 3), (2, 1, 5), (3, 7, 65), (2, 513, 2), (8, 100, 33), (8, 2048, 2)],
    "dups": [(3, 7, 65), (2, 511, 2), (2, 512, 2), (2, 513, 2), (5, 257, 4), (8, 100, 33), (7, 2340, 1),
             (4, 300, 1000)] + LDS_EDGE,
}
TIE_POOL = np.array([0x3f800000, 0x3f800001, 0x40490fdb], dtype=np.uint32)      # 1.0, the float after it, pi
PAD_KEY = np.uint64(0xffffffffffffffff)
ID_MAX = 2**31 - 1
SENTINEL_ID, SENTINEL_BITS = 0x5a5a5a5a, 0x7fc12345        # what a GPU test pre-fills its outputs with (a NaN)


def make_case(n_lists, top_k, nq, fill, seed):
    return dict(n_lists=n_lists, top_k=top_k, nq=nq, fill=fill, seed=seed)


def case_id(c):
    return "L%d_k%d_nq%d_%s_s%d" % (c["n_lists"], c["top_k"], c["nq"], c["fill"], c["seed"])


def _build_table():
    out = []
    for f, (fill, shapes) in enumerate(FILLS.items()):
        for s, (n_lists, top_k, nq) in enumerate(shapes):
            out.append(make_case(n_lists, top_k, nq, fill, 1000 * (f + 1) + s))
    return out


TABLE = _build_table()


# ---- keys ---------------------------------------------------------------------------------------------------------------

def bits_of(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def keys_of(ids, dists):
    """uint64 `distance bits << 32 | id` of valid rows, PAD_KEY of padding rows: what the kernel holds in LDS."""
    ids = np.asarray(ids)
    k = (bits_of(dists).astype(np.uint64) << np.uint64(32)) | (ids.astype(np.int64) & 0xffffffff).astype(np.uint64)
    return np.where(ids >= 0, k, PAD_KEY)


def _distinct_ids(rng, count):
    """`count` distinct ids below 2^31, unordered."""
    out = np.unique(rng.integers(0, ID_MAX, size=count + count // 8 + 8, dtype=np.int64))
    while len(out) < count:
        out = np.unique(np.concatenate((out, rng.integers(0, ID_MAX, size=count, dtype=np.int64))))
    return rng.permutation(out)[:count]


def _positive(rng, count):
    """float32 distances in [2^-10, 2^10), as bit patterns."""
    return np.exp2(rng.uniform(-10, 10, size=count)).astype(np.float32).view(np.uint32)


def _deal(rng, n_lists, top_k, total):
    """The list of each of `total` rows: uniformly, no list beyond top_k rows."""
    assert total <= n_lists * top_k
    return rng.permutation(np.repeat(np.arange(n_lists), top_k))[:total]


def _plain_padding(rng, count):
    return np.full(count, -1, dtype=np.int64), np.full(count, 0x7f800000, dtype=np.uint32)


def _odd_padding(rng, count):
    ids = rng.choice(np.array([-1, -2, -2**31, 0], dtype=np.int64), size=count)
    ids = np.where(ids == 0, -rng.integers(1, 2**31, size=count, dtype=np.int64), ids)
    menu = np.array([0x00000000, 0xbf800000, 0x7fc00000, 0x7f800000, 1], dtype=np.uint32)
    b = rng.choice(menu, size=count)
    return ids, np.where(b == 1, _positive(rng, count), b)


def _place(ids, dists, q, owner, row_bits, row_ids, rng, padding=_plain_padding):
    """Write query q: list l gets the rows with owner == l, ascending by (bits, id), then padding."""
    n_lists, _, top_k = ids.shape
    for l in range(n_lists):
        sel = np.flatnonzero(owner == l)
        sel = sel[np.lexsort((row_ids[sel], row_bits[sel]))]
        assert len(sel) <= top_k
        pi, pb = padding(rng, top_k - len(sel))
        ids[l, q] = np.concatenate((row_ids[sel], pi))
        dists[l, q] = np.concatenate((row_bits[sel], pb)).astype(np.uint32).view(np.float32)


def _fill_query(c, q, rng, ids, dists):
    L, k, fill = c["n_lists"], c["top_k"], c["fill"]
    n = L * k
    padding = _plain_padding
    if fill == "full":
        owner = _deal(rng, L, k, n)
        row_ids, row_bits = _distinct_ids(rng, n), _positive(rng, n)
    elif fill == "ragged":
        counts = rng.integers(0, k + 1, size=L)
        e, f = rng.choice(L, size=2, replace=False)
        counts[e], counts[f] = 0, k
        owner = np.repeat(np.arange(L), counts)
        row_ids, row_bits = _distinct_ids(rng, len(owner)), _positive(rng, len(owner))
    elif fill == "short":
        total = int(rng.integers(1, k)) if k > 1 else 0
        owner = _deal(rng, L, k, total)
        row_ids, row_bits = _distinct_ids(rng, total), _positive(rng, total)
    elif fill == "all_empty":
        owner = np.zeros(0, dtype=np.int64)
        row_ids, row_bits = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32)
    elif fill == "ties":
        owner = _deal(rng, L, k, n)
        row_ids = _distinct_ids(rng, n)
        row_bits = np.full(n, TIE_POOL[1]) if q == 0 else TIE_POOL[rng.integers(0, 3, size=n)]
    elif fill == "interleaved":
        row_ids, row_bits = _distinct_ids(rng, n), _positive(rng, n)
        order = np.lexsort((row_ids, row_bits))
        owner = np.empty(n, dtype=np.int64)
        owner[order] = np.arange(n) % L
    elif fill in ("one_wins_first", "one_wins_last"):
        row_ids, row_bits = _distinct_ids(rng, n), _positive(rng, n)
        order = np.lexsort((row_ids, row_bits))
        others = np.array([l for l in range(L) if l != (0 if fill == "one_wins_first" else L - 1)])
        owner = np.empty(n, dtype=np.int64)
        owner[order[:k]] = 0 if fill == "one_wins_first" else L - 1
        owner[order[k:]] = rng.permutation(np.repeat(others, k))
    elif fill == "edges_of_value":
        padding = _odd_padding
        n_fin = min(k // 2, n)
        n_inf = min(k // 2 + 2 if L > 1 else k // 4 + 1, n - n_fin)       # (one list: room for padding rows)
        row_ids = _distinct_ids(rng, n_fin + n_inf)
        row_bits = np.concatenate((_positive(rng, n_fin), np.full(n_inf, 0x7f800000, dtype=np.uint32)))
        row_bits[:(n_fin + 2) // 3] = 0                   # 0.0
        row_ids[0] = ID_MAX                               # (top_k = 1 has no finite row: then on the first +inf row)
        if len(row_ids) > 1:
            row_ids[-1] = 0
        owner = _deal(rng, L, k, n_fin + n_inf)
    elif fill == "dups":
        assert L >= 2 and k >= 2
        kind = q % 3
        n_rep = 1 if kind == 2 else int(rng.integers(1, max(2, k // 2)))       # the repeated rows, the query's smallest
        rep_ids = _distinct_ids(rng, n_rep)
        rep_bits = np.sort(np.exp2(rng.uniform(-14, -11, size=n_rep)).astype(np.float32).view(np.uint32))
        if kind == 0:
            holders = [0, 1]
        elif kind == 1:
            holders = list(range(L))
        else:
            holders = [0, 0, L - 1]
        room = np.full(L, k)
        for l in holders:
            room[l] -= n_rep
        fill_owner = rng.permutation(np.repeat(np.arange(L), room))
        fill_owner = fill_owner[:int(rng.integers(len(fill_owner) // 2, len(fill_owner) + 1))]
        owner = np.concatenate([np.full(n_rep, l) for l in holders] + [fill_owner])
        row_ids = np.concatenate([rep_ids] * len(holders) + [_distinct_ids(rng, len(fill_owner))])
        row_bits = np.concatenate([rep_bits] * len(holders) + [_positive(rng, len(fill_owner))])
    else:
        raise ValueError(fill)
    _place(ids, dists, q, np.asarray(owner, dtype=np.int64), np.asarray(row_bits, dtype=np.uint32),
           np.asarray(row_ids, dtype=np.int64), rng, padding)


@functools.lru_cache(maxsize=None)
def _built(key):
    n_lists, top_k, nq, fill, seed = key
    c = make_case(n_lists, top_k, nq, fill, seed)
    rng = np.random.default_rng([seed, n_lists, top_k, nq])
    ids = np.empty((n_lists, nq, top_k), dtype=np.int32)
    dists = np.empty((n_lists, nq, top_k), dtype=np.float32)
    for q in range(nq):
        _fill_query(c, q, rng, ids, dists)
    want = reference(ids, dists)
    for a in (ids, dists) + want:
        a.setflags(write=False)
    return ids, dists, want


def build_lists(c):
    """(ids, dists, (want_ids, want_dists)) of a case: the lists and their reference, built once and read-only."""
    return _built((c["n_lists"], c["top_k"], c["nq"], c["fill"], c["seed"]))


# ---- the reference --------------------------------------------------------------------------------------------------------

def reference(ids, dists):
    """Merged (ids int32 [nq][top_k], dists float32 [nq][top_k]) of lists [n_lists][nq][top_k]."""
    ids, b = np.asarray(ids), bits_of(dists)
    _, nq, top_k = ids.shape
    out_i = np.full((nq, top_k), -1, dtype=np.int32)
    out_b = np.full((nq, top_k), 0x7f800000, dtype=np.uint32)
    for q in range(nq):
        qi, qb = ids[:, q].reshape(-1), b[:, q].reshape(-1)
        valid = qi >= 0
        qi, qb = qi[valid], qb[valid]
        order = np.lexsort((qi, qb))[:top_k]
        out_i[q, :len(order)] = qi[order]
        out_b[q, :len(order)] = qb[order]
    return out_i, out_b.view(np.float32)


# ---- the kernel's rank rule, restated -----------------------------------------------------------------------------------

def rank_rule(ids, dists, stable):
    """What merge_kernel writes, from its own rule: the output starts as padding; the key at position p of list `own`
    goes to rank p + sum over the other lists of a binary search (np.searchsorted) for it, if that is below top_k.
    stable = False: the search counts the keys strictly below it in every other list (the rule the kernel had).
    stable = True: keys <= it in the lists before `own`, keys < it in the lists after (the rule it has)."""
    n_lists, nq, top_k = np.asarray(ids).shape
    keys = keys_of(ids, dists)
    out_i = np.full((nq, top_k), -1, dtype=np.int32)
    out_b = np.full((nq, top_k), 0x7f800000, dtype=np.uint32)
    for q in range(nq):
        K = keys[:, q]                                                  # [n_lists][top_k], every row ascending
        own, pos = np.nonzero(K != PAD_KEY)                             # list by list: `own` ascends
        mine = K[own, pos]
        rank = pos.astype(np.int64)
        first, last = np.searchsorted(own, np.arange(n_lists), "left"), np.searchsorted(own, np.arange(n_lists), "right")
        for l in range(n_lists if len(mine) else 0):
            a, b = first[l], last[l]                                    # mine[a:b] are list l's own keys
            rank[:a] += np.searchsorted(K[l], mine[:a], side="left")    # l comes after their list
            rank[b:] += np.searchsorted(K[l], mine[b:], side="right" if stable else "left")     # l comes before it
        keep = rank < top_k
        out_i[q, rank[keep]] = (mine[keep] & np.uint64(0xffffffff)).astype(np.int64)
        out_b[q, rank[keep]] = (mine[keep] >> np.uint64(32)).astype(np.uint32)
    return out_i, out_b.view(np.float32)


def has_hole(got_ids, want_ids):
    """A padding row where the reference holds a valid one."""
    return bool(np.any((np.asarray(got_ids) < 0) & (np.asarray(want_ids) >= 0)))


def ties_straddle(ids, dists, q):
    """The tie condition of the module docstring for query q."""
    ids, b = np.asarray(ids), bits_of(dists)
    n_lists, _, top_k = ids.shape
    qi, qb = ids[:, q].reshape(-1), b[:, q].reshape(-1)
    lst = np.repeat(np.arange(n_lists), top_k)
    valid = qi >= 0
    qi, qb, lst = qi[valid], qb[valid], lst[valid]
    order = np.lexsort((qi, qb))
    if len(order) <= top_k or qb[order[top_k - 1]] != qb[order[top_k]]:
        return False
    tie = qb[order] == qb[order[top_k]]
    kept, cut = set(lst[order[:top_k]][tie[:top_k]].tolist()), set(lst[order[top_k:]][tie[top_k:]].tolist())
    return len(kept | cut) >= 2
