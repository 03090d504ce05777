"""IVF search (dpq_ivf_*) at the edges its first suite (tests/test_ivf_search.py) does not reach: calls cut into query
slices, merges of many rounds, the probe pre-pass beyond one stride of threads, the width of the list build's sort, the
scan's threshold on lists in distance order, the five numeric classes left out there, the assignment by centroids in more
than one step.

Every comparison is strict -- ids equal, distances equal as fp32 bit patterns, padding -1 / +inf -- against
tests/_ivf_restatement.py over the exact-rational distances of tests/_numeric_edges.py, and against query_batch on the
same handle wherever every node is labelled and every list probed.  Nothing is skipped and no case is exempt.

Choices the issue leaves open, and why:
 * "order inside a list" uses one query, the all-zero one, and FOUR lists of 9000 nodes over an index of 36 001: row q of
   the call probes list q, whose distances descend with the position in the list (q = 0), ascend (1), are all equal (2)
   and descend in runs of 300 ties (3); a fifth row probes all four.  The scan sees exactly the orders the issue asks
   for, and the table stays the table by construction (any other query would put roundings into it).
 * its table: T[0][a] = ceil(sqrt(70 000 a))^2 and T[1][b] = b^2.  256 c^2 and c^2 / 256 need 27 bits at 9000 nodes and
   would tie after rounding; these sums are whole numbers below 2^22, exact under both accumulate rules, and a step of
   T[0] (more than 66 000) outweighs all of T[1] (at most 65 025), so the distance is strictly monotone in 256 a + b.
 * the probe rows of width 256 have no entry 256: there entry 0 recurs at 255.
"""
import numpy as np
import pytest

import _ivf_restatement as R
import _numeric_edges as ne
import _option_matrix as om

ERR_ARG = -1
_cache = {}


def built_class(name, M=8, n=ne.N_SCAN):
    """One build per (class, M, n) and module; nobody writes to it."""
    key = (name, M, n)
    if key not in _cache:
        _cache[key] = ne.build_class(name, M, 256, n, plain_rule=True)
    return _cache[key]


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def open_class(api, c, plain=False, **opts):
    if plain:
        idx = api.DeltaPQIndex.open_plain(c["codes"], K=c["K"], **opts)
    else:
        idx = api.DeltaPQIndex.open_memory(c["payload"], c["n"], c["M"], c["K"], **opts)
    return idx.set_codebook(c["cb"])


def queries_of(c, nq):
    use = np.arange(nq) % len(c["queries"])
    return use, np.ascontiguousarray(c["queries"][use])


def labels_of(n, nlist, seed, unassigned=0.0):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, nlist, size=n).astype(np.int32)
    if unassigned:
        labels[rng.random(n) < unassigned] = -1
    return labels


def prefixes(nq, nlist, nprobe, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int32)


def no_id_twice(ids, what):
    for q, row in enumerate(ids):
        real = row[row >= 0]
        assert len(np.unique(real)) == len(real), "%s query %d: an id is reported twice" % (what, q)


def refused_in_the_last_slice(api, ivf, qs, probes, nlist, k, want, what):
    """A probe >= nlist in the LAST row only, through the device form: DPQ_ERR_ARG, and the next call answers as before."""
    import torch
    bad = probes.copy()
    bad[-1, -1] = nlist
    t_q = torch.from_numpy(qs).cuda()
    with pytest.raises(api.DpqError) as e:
        ivf.search_probes_torch(t_q, torch.from_numpy(bad).cuda(), k)
    assert e.value.status == ERR_ARG, what
    i, d = ivf.search_probes_torch(t_q, torch.from_numpy(probes).cuda(), k)
    om._rows_equal((i.cpu().numpy(), d.cpu().numpy()), want, what + ", device form after the refused call")


# ---- CPU: the arithmetic the shapes below rest on -----------------------------------------------------------------------------

def slices_of(nq, nprobe, top_k):
    """(per, round) of include/deltapq_amd.h's limits: 2048 queries and 256 MiB of partial answers per slice, 16 384 keys
    per merge."""
    per = max(1, min(nq, 2048, (256 << 20) // (nprobe * top_k * 8)))
    return per, 16384 // top_k


def test_the_shapes_cross_the_edges_they_are_chosen_for():
    assert slices_of(2049, 2, 3) == (2048, 5461) and slices_of(4097, 2, 3)[0] == 2048 and 4097 - 2 * 2048 == 1
    assert slices_of(33, 1024, 2048) == (16, 8) and 33 - 2 * 16 == 1
    assert slices_of(160, 300, 700) == (159, 23)
    rounds = {(k, p): slices_of(5, p, k)[1] for k, p in MERGE_CALLS}
    assert rounds[(2048, 8)] == 8 and rounds[(2048, 9)] == 8                         # nprobe == round, round + 1
    assert rounds[(17, 963)] == 963 and rounds[(17, 964)] == 963 and 963 & 962       # ... a round that is no power of two
    assert rounds[(1500, 10)] == 10 and rounds[(1500, 11)] == 10
    assert rounds[(2047, 1024)] == 8                                                 # 1 + ceil(1016 / 7) = 147 rounds
    T, codes, labels = order_case(8)[1:4]
    d = ne.exact_distances(T, codes)
    assert np.array_equal(bits(d), bits(ne.exact_distances_fp32_rule(T, codes))) and d.max() < 2 ** 22
    for l, (lo_ok, hi_ok) in enumerate(((True, False), (False, True), (True, True), (True, False))):
        step = np.diff(d[labels == l].astype(np.float64))
        assert (labels == l).sum() == ORDER_LEN and np.all(step <= 0) == lo_ok and np.all(step >= 0) == hi_ok, l
    assert np.all(np.diff(d[labels == 0]) < 0) and np.all(np.diff(d[labels == 1]) > 0)  # strictly
    runs = np.flatnonzero(np.diff(d[labels == 3]) != 0) + 1
    assert np.array_equal(runs, np.arange(300, ORDER_LEN, 300))


# ---- 1. query slices --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nq", [2049, 4097])
def test_slices_of_2048_queries(gpu, nq):
    """n = 4097, nlist 7, nprobe 2, top_k 3: slices of 2048 (, 2048) and 1 query."""
    c = built_class("fp32_ties")
    n, nlist, k = c["n"], 7, 3
    labels = labels_of(n, nlist, 101, unassigned=0.05)
    rng = np.random.default_rng(102)
    probes = rng.integers(-1, nlist, size=(nq, 2)).astype(np.int32)
    probes[-1] = [3, 5]
    use, qs = queries_of(c, nq)
    offsets, ids = R.lists_from_labels(labels, nlist)
    want = R.search(c["d64"], use, offsets, ids, probes, k)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        om._rows_equal(ivf.search_probes(qs, probes, k), want, "nq %d" % nq)
        refused_in_the_last_slice(gpu, ivf, qs, probes, nlist, k, want, "nq %d" % nq)
        om._rows_equal(ivf.search_probes(qs, probes, k), want, "nq %d, after the refused call" % nq)
        with gpu.IVF.from_labels(idx, np.abs(labels), nlist) as full:
            every = prefixes(nq, nlist, nlist, 103)
            assert same(full.search_probes(qs, every, k), idx.query_batch(qs, k)), "nq %d: differs from query_batch" % nq


@pytest.mark.gpu
def test_slices_of_sixteen_queries_and_147_rounds(gpu):
    """n = 20 001, nlist = nprobe = 1024, top_k = 2048, nq = 33: slices of 16, 16 and 1 query, each merged in rounds of 8
    lists."""
    c = built_class("fp32_ties", 8, 20001)
    n, nlist, k, nq = c["n"], 1024, 2048, 33
    labels = labels_of(n, nlist, 111)
    probes = prefixes(nq, nlist, nlist, 112)
    use, qs = queries_of(c, nq)
    want = [ne.topk(c["d64"][u], k) for u in use]
    offsets, ids = R.lists_from_labels(labels, nlist)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        got = ivf.search_probes(qs, probes, k)
        om._rows_equal(got, want, "33 queries, 1024 lists")
        om._rows_equal((got[0][-1:], got[1][-1:]), R.search(c["d64"], use[-1:], offsets, ids, probes[-1:], k),
                       "the last slice against the restatement")
        assert same(got, idx.query_batch(qs, k)), "differs from query_batch"
        refused_in_the_last_slice(gpu, ivf, qs, probes, nlist, k, want, "33 queries, 1024 lists")


@pytest.mark.gpu
def test_slices_of_159_queries(gpu):
    """nprobe 300, top_k 700, nq = 160: a slice of 159 and one of 1, rounds of 23 lists."""
    c = built_class("fp32_ties", 8, 20001)
    n, nlist, nprobe, k, nq = c["n"], 1024, 300, 700, 160
    labels = labels_of(n, nlist, 121, unassigned=0.05)
    probes = prefixes(nq, nlist, nprobe, 122)
    probes[7, 100:120] = -1
    probes[nq - 1, 299] = probes[nq - 1, 4]
    use, qs = queries_of(c, nq)
    offsets, ids = R.lists_from_labels(labels, nlist)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        got = ivf.search_probes(qs, probes, k)
        om._rows_equal(got, R.search(c["d64"], use, offsets, ids, probes, k), "160 queries, 300 lists")
        no_id_twice(got[0], "160 queries, 300 lists")


# ---- 2. merge rounds -----------------------------------------------------------------------------------------------------------

MERGE_CALLS = [(2048, 8), (2048, 9), (17, 963), (17, 964), (17, 1024), (1500, 10), (1500, 11), (2047, 1024)]


@pytest.mark.gpu
def test_merge_rounds(gpu):
    c = built_class("fp32_ties", 8, 20001)
    n, nlist, nq = c["n"], 1024, 5
    labels = labels_of(n, nlist, 131)
    use, qs = queries_of(c, nq)
    offsets, ids = R.lists_from_labels(labels, nlist)
    with open_class(gpu, c) as idx:
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            for j, (k, nprobe) in enumerate(MERGE_CALLS):
                probes = prefixes(nq, nlist, nprobe, 140 + j)
                got = ivf.search_probes(qs, probes, k)
                om._rows_equal(got, R.search(c["d64"], use, offsets, ids, probes, k), "top-%d of %d lists" % (k, nprobe))
                if nprobe == nlist:
                    assert same(got, idx.query_batch(qs, k)), "top-%d of every list: differs from query_batch" % k
        # a call with rounds after a smaller call on a fresh structure: every buffer grows, the rounds' own appear
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            probes = prefixes(nq, nlist, 2, 150)
            om._rows_equal(ivf.search_probes(qs, probes, 10), R.search(c["d64"], use, offsets, ids, probes, 10), "top-10 of 2 lists")
            probes = prefixes(nq, nlist, nlist, 151)
            got = ivf.search_probes(qs, probes, 2048)
            om._rows_equal(got, [ne.topk(c["d64"][u], 2048) for u in use], "top-2048 of 1024 lists after a small call")
            assert same(got, idx.query_batch(qs, 2048))


# ---- 3. the probe pre-pass -------------------------------------------------------------------------------------------------------

def prepass_rows(nlist, w, seed):
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.permutation(nlist)[:w] for _ in range(7)]).astype(np.int32)
    for at in (255 if w == 256 else 256, 257, 1023):       # entry 0 again, in the same and in later strides
        if at < w:
            rows[0, at] = rows[0, 0]
    if w > 800:
        rows[1, 800] = rows[1, 300]                         # second stride, again in the fourth
        rows[1, 900] = rows[1, 600]
    rows[2, 250:min(w, 261)] = -1                           # a run of padding across 255 / 256
    rows[3, :] = rows[3, 0]                                 # one list, w times
    rows[4, :] = -1
    rows[5, 1::2] = rows[5, 0:w - 1:2][:len(rows[5, 1::2])]  # every entry twice, side by side
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("w", [256, 257, 1024])
def test_probe_rows_of_more_than_one_stride(gpu, w):
    c = built_class("fp32_ties", 8, 20001)
    n, nlist = c["n"], 1024
    labels = labels_of(n, nlist, 161, unassigned=0.05)
    probes = prepass_rows(nlist, w, 162 + w)
    use, qs = queries_of(c, len(probes))
    offsets, ids = R.lists_from_labels(labels, nlist)
    with open_class(gpu, c) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        for k in (60, 2048):
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, R.search(c["d64"], use, offsets, ids, probes, k), "rows of %d top-%d" % (w, k))
            no_id_twice(got[0], "rows of %d top-%d" % (w, k))
            assert np.all(got[0][4] == -1) and np.all(np.isposinf(got[1][4])), "the row of padding"
            assert (got[0][3] >= 0).sum() == min(k, offsets[probes[3, 0] + 1] - offsets[probes[3, 0]]), "one list, %d times" % w


# ---- 4. the sort width of the list build ----------------------------------------------------------------------------------------

def check_structure(ivf, labels, nlist, what):
    offsets, ids = R.lists_from_labels(labels, nlist)
    got = ivf.lists()
    assert np.array_equal(got[0], offsets), what + ": offsets"
    assert np.array_equal(got[1], ids), what + ": ids"
    inf = ivf.info()
    assert (inf["nlist"], inf["n_assigned"], inf["n_unassigned"], inf["max_list_len"]) == \
        (nlist, (labels >= 0).sum(), (labels < 0).sum(), np.diff(offsets).max()), "%s: %s" % (what, inf)
    return offsets, ids


@pytest.mark.gpu
@pytest.mark.parametrize("nlist", [1, 2, 256, 4096, 65536])
def test_unassigned_nodes_and_the_last_list(gpu, nlist):
    """Key nlist (the unassigned node) needs a bit more than the largest label exactly when nlist is a power of two."""
    import torch
    c = built_class("fp32_ties", 8, 20001)
    n, nq, k = c["n"], 5, 300
    labels = labels_of(n, nlist, 171, unassigned=0.10)
    labels[[5, n - 1]] = nlist - 1
    assert (labels < 0).sum() > 1500 and labels.max() == nlist - 1
    nprobe = min(nlist, 1024)
    rng = np.random.default_rng(172)
    probes = np.stack([np.concatenate([[nlist - 1], rng.permutation(nlist - 1)[:nprobe - 1]]) for _ in range(nq)]).astype(np.int32)
    use, qs = queries_of(c, nq)
    with open_class(gpu, c) as idx:
        for name, lab in (("host labels", labels), ("device labels", torch.from_numpy(labels).cuda())):
            with gpu.IVF.from_labels(idx, lab, nlist) as ivf:
                offsets, ids = check_structure(ivf, labels, nlist, "nlist %d, %s" % (nlist, name))
                got = ivf.search_probes(qs, probes, k)
                om._rows_equal(got, R.search(c["d64"], use, offsets, ids, probes, k), "nlist %d, %s" % (nlist, name))


@pytest.mark.gpu
def test_65536_lists_with_every_node_in_the_last_and_with_none_in_any(gpu):
    c = built_class("fp32_ties", 8, 20001)
    n, nq, nlist = c["n"], 5, 65536
    use, qs = queries_of(c, nq)
    probes = np.tile(np.array([17, 65535, -1, 0], dtype=np.int32), (nq, 1))
    with open_class(gpu, c) as idx:
        labels = np.full(n, nlist - 1, dtype=np.int32)
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            offsets, ids = check_structure(ivf, labels, nlist, "every node in list 65535")
            assert offsets[nlist - 1] == 0 and offsets[nlist] == n and np.array_equal(ids, np.arange(n))
            for k in (10, 2048):
                got = ivf.search_probes(qs, probes, k)
                om._rows_equal(got, [ne.topk(c["d64"][u], k) for u in use], "every node in list 65535 top-%d" % k)
                assert same(got, idx.query_batch(qs, k))
        labels = np.full(n, -1, dtype=np.int32)
        with gpu.IVF.from_labels(idx, labels, nlist) as ivf:
            check_structure(ivf, labels, nlist, "every node unassigned")
            assert ivf.info()["n_assigned"] == 0 and ivf.info()["max_list_len"] == 0
            got = ivf.search_probes(qs, probes, 10)
            assert np.all(got[0] == -1) and np.all(np.isposinf(got[1])), "every search is all padding"


# ---- 5. order inside a list ---------------------------------------------------------------------------------------------------------

ORDER_LEN, ORDER_RUN = 9000, 300


def order_case(M):
    """(cb, T, codes [36 001][M], labels, tree): see the module docstring.  Node 0 is in no list."""
    key = ("order", M)
    if key in _cache:
        return _cache[key]
    n = 4 * ORDER_LEN + 1
    J = np.full((M, 256), 3, dtype=np.int64)
    J[0] = 0
    J[0, :36] = np.ceil(np.sqrt(70000.0 * np.arange(36))).astype(np.int64)
    J[1] = np.arange(256)
    assert np.all(np.diff(J[0, :36] ** 2) > 255 ** 2)
    rng = np.random.default_rng(181)
    labels = np.full(n, -1, dtype=np.int32)
    labels[1:] = rng.permutation(np.repeat(np.arange(4, dtype=np.int32), ORDER_LEN))
    value = np.zeros(n, dtype=np.int64)
    p = np.arange(ORDER_LEN)
    for l, v in enumerate((ORDER_LEN - 1 - p, p, np.full(ORDER_LEN, 4321), (ORDER_LEN - 1 - p) // ORDER_RUN)):
        value[labels == l] = v
    codes = np.full((n, M), 7, dtype=np.uint8)
    codes[:, 0], codes[:, 1] = value >> 8, value & 255
    depths = np.ones(n, dtype=np.uint8)
    depths[0] = 0
    change = np.zeros((n, M), dtype=bool)
    change[:, :2] = True
    tree = ne.tree_from_parts(codes[0], depths, change, codes, M)
    _cache[key] = (ne.grid_codebook(J, 0), ne.table_by_construction(J, 0), codes, labels, tree)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("plain", [False, True], ids=["dtc", "plain"])
@pytest.mark.parametrize("M", [8, 16])
def test_lists_in_distance_order(gpu, M, plain):
    from deltapq_amd import synth
    cb, T, codes, labels, tree = order_case(M)
    n = len(codes)
    assert np.array_equal(synth.decode_tree_codes(tree), codes) and ne.table_by_the_book(cb, np.zeros(M, dtype=np.float32)) == T
    d = (ne.exact_distances_fp32_rule if plain else ne.exact_distances)(T, codes)[None, :]
    probes = np.array([[0, -1, -1, -1], [1, -1, -1, -1], [2, -1, -1, -1], [3, -1, -1, -1], [2, 0, 3, 1]], dtype=np.int32)
    use = np.zeros(len(probes), dtype=np.int64)
    qs = np.zeros((len(probes), M), dtype=np.float32)
    offsets, ids = R.lists_from_labels(labels, 4, even_rule=not plain)
    if plain:
        idx = gpu.DeltaPQIndex.open_plain(codes, K=256)
    else:
        idx = gpu.DeltaPQIndex.open_memory(synth.encode_dtc(tree)[0], n, M, 256)
    with idx, gpu.IVF.from_labels(idx.set_codebook(cb), labels, 4) as ivf:
        assert np.array_equal(ivf.lists()[1], ids)
        for k in (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048):
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, R.search(d, use, offsets, ids, probes, k, even_rule=not plain), "M %d top-%d" % (M, k))
        assert got[0][0][0] == ids[offsets[1] - 1] and got[0][1][0] == ids[offsets[1]]   # the last of list 0, the first of list 1
        assert np.array_equal(got[0][2], ids[offsets[2]:offsets[2] + 2048])              # all equal: by id


# ---- 6. the numeric classes the first suite leaves out ---------------------------------------------------------------------------

HANDLES = {"dtc_m8": (8, False), "dtc_m16": (16, False), "plain_m8": (8, True), "plain_m16": (16, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", ["zero_threshold", "ladder_low", "ladder_mid", "ladder_high", "tiny_gaussian"])
def test_every_list_probed_is_the_exhaustive_search(gpu, name, handle):
    M, plain = HANDLES[handle]
    c = built_class(name, M)
    n = c["n"]
    alld = c["d32"] if plain else c["d64"]
    nq, nlist = 5, 7
    use, qs = queries_of(c, nq)
    labels = labels_of(n, nlist, n + M)
    probes = prefixes(nq, nlist, nlist, n + M + 1)
    with open_class(gpu, c, plain) as idx, gpu.IVF.from_labels(idx, labels, nlist) as ivf:
        for k in (1, 10, 257):
            what = "%s %s top-%d" % (name, handle, k)
            got = ivf.search_probes(qs, probes, k)
            om._rows_equal(got, [ne.topk(alld[u], k) for u in use], what)
            assert same(got, idx.query_batch(qs, k)), what + ": differs from query_batch on this handle"


# ---- 7. the assignment in more than one step ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [False, True], ids=["one_tile", "tiles_of_600"])
def test_assignment_steps(gpu, tiled, monkeypatch):
    """n = 65 536 + 1300: two assignment steps of 65 536 nodes, each in query batches of 1024; with decode tiles of 600
    nodes (the developer hook) tiles, steps and batches all cross each other."""
    from deltapq_amd import synth
    n, M, Ds, nlist = 65536 + 1300, 8, 4, 5
    tree = ne.plain_tree(n, M, 256, 191)
    payload, _ = synth.encode_dtc(tree)
    cb = synth.make_codebook(M, 256, Ds, 192)
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as idx:
        idx.set_codebook(cb)
        recon = idx.reconstruct(R.reported_ids(0, n))
        codes = synth.decode_tree_codes(tree)
        assert np.array_equal(recon, cb[np.arange(M)[None, :], codes].reshape(n, M * Ds))
        rng = np.random.default_rng(193)
        cents = recon[rng.choice(n, size=nlist, replace=False)] + rng.normal(size=(nlist, M * Ds)).astype(np.float32) * 20
        cents[3] = cents[1]                                                      # two exact duplicates: list 3 stays empty
        labels = R.assign(recon, cents)
        counts = np.bincount(labels, minlength=nlist)
        assert counts[3] == 0 and np.all(np.delete(counts, 3) > 0)
        assert len(np.unique(labels[65536:])) > 1 and len(np.unique(labels[:1024])) > 1
        offsets, ids = R.lists_from_labels(labels, nlist)
        if tiled:
            monkeypatch.setenv("DPQ_DEV", "1")
            monkeypatch.setenv("DPQ_IVF_TILE_NODES", "600")
        with gpu.IVF.build(idx, cents) as ivf:
            got = ivf.lists()
            assert np.array_equal(got[0], offsets), "offsets: %s, expected %s" % (got[0], offsets)
            assert np.array_equal(got[1], ids)
