"""DeltaTree builder (host), codes.bin.plain / TreeNodesDFS files,
PQ encoder (GPU) -- the callers either side of the query path."""
import os

import numpy as np
import pytest


def clustered_codes(n, M=8, seed=0, n_protos=None):
    """PQ-code-like data: prototypes + few-position perturbations + exact duplicates."""
    rng = np.random.default_rng(seed)
    n_protos = n_protos or max(4, n // 50)
    protos = rng.integers(0, 256, size=(n_protos, M), dtype=np.uint8)
    codes = protos[rng.integers(0, n_protos, size=n)].copy()
    nchg = rng.integers(0, 4, size=n)
    for i in range(n):
        for pos in rng.choice(M, nchg[i], replace=False):
            codes[i, pos] = rng.integers(0, 256)
    return codes


def tree_decode(tree):
    """Codes of every DFS position from the builder's arrays."""
    from deltapq_amd import synth
    t = dict(root=tree.root, depths=tree.depth, masks=tree.mask, deltas=tree.deltas, M=tree.M)
    return synth.decode_tree_codes(t)


@pytest.mark.parametrize("n,M", [(1, 8), (2, 8), (3, 8), (500, 8), (20000, 8), (3000, 16)])
def test_builder_is_lossless_and_valid(lib, oracle, n, M):
    from deltapq_amd import api
    codes = clustered_codes(n, M, seed=n)
    tree = api.DeltaTree(codes, K=256, max_height_folds=1)
    assert sorted(tree.vec_id.tolist()) == list(range(n))             # a permutation: every code exactly once
    assert np.array_equal(tree_decode(tree), codes[tree.vec_id])      # lossless
    assert tree.depth[0] == 0 and (n == 1 or tree.depth[1:].min() >= 1)
    assert tree.stats["max_depth"] <= (7 if M <= 8 else 15)           # height cap M*h keeps the 3-bit depth field valid
    assert np.all(tree.depth[1:].astype(int) <= tree.depth[:-1].astype(int) + 1)   # DFS layout
    assert len(tree.edges) == n - 1
    if n > 1:
        par = tree.parent_pos[1:]
        assert np.all(par < np.arange(1, n)) and np.all(tree.depth[1:] == tree.depth[par] + 1)
    # masks are exactly the differing positions w.r.t. the parent
    if n > 1:
        child, parent = codes[tree.vec_id[1:]], codes[tree.vec_id[tree.parent_pos[1:]]]
        bits = ((child != parent) * (1 << np.arange(M))).sum(1)
        assert np.array_equal(bits.astype(np.uint16), tree.mask[1:])
    payload = tree.payload()
    st = api.dtc_validate(payload, n, M)
    assert st["n_diffs"] == tree.stats["n_diffs"] and len(payload) == tree.stats["n_bytes"]
    lut = np.random.default_rng(1).random((M, 256)).astype(np.float32)
    _, _, _, allc = oracle.scan_lut(payload, n, lut, 1, want_all=True)
    assert np.array_equal(allc, codes[tree.vec_id])                   # the oracle's scan decodes the same codes


def test_builder_exploits_similarity(lib):
    """Duplicates become 0-diff children and near-duplicates 1-3-diff children: far fewer
    changed bytes than M per code (the point of DeltaPQ)."""
    from deltapq_amd import api
    n = 30000
    codes = clustered_codes(n, 8, seed=3, n_protos=300)
    tree = api.DeltaTree(codes)
    assert tree.stats["n_diffs"] < 2.5 * n
    assert tree.stats["n_bytes"] < 0.55 * 8 * n                       # < 55 % of raw PQ
    assert (tree.mask[1:] == 0).sum() >= n - len(np.unique(codes, axis=0)) - 1
    rnd = np.random.default_rng(0).integers(0, 256, size=(n, 8), dtype=np.uint8)
    assert api.DeltaTree(rnd).stats["n_diffs"] > tree.stats["n_diffs"] * 2   # random codes compress worse


def test_sibling_order_uses_codebook(lib, codebook):
    from deltapq_amd import api
    codes = clustered_codes(5000, 8, seed=5)
    a, b = api.DeltaTree(codes), api.DeltaTree(codes, codebook=codebook)
    assert np.array_equal(np.sort(a.edges.view([("p", "u4"), ("c", "u4")]).ravel()),
                          np.sort(b.edges.view([("p", "u4"), ("c", "u4")]).ravel()))   # same tree ...
    assert not np.array_equal(a.vec_id, b.vec_id)                                      # ... other sibling order
    assert np.array_equal(tree_decode(b), codes[b.vec_id])


def test_reference_artefact_files(lib, tmp_path, codebook):
    from deltapq_amd import api, synth
    d = str(tmp_path)
    n = 4001
    codes = clustered_codes(n, 8, seed=7)
    path = os.path.join(d, "codes.bin.plain.M8K256N%d" % n)
    api.write_codes_plain(path, codes)
    assert os.path.getsize(path) == 8 + n * 8                          # int64 N + N*M bytes (pq_tree.cpp:1011-1031)
    assert np.array_equal(api.read_codes_plain(path, 8), codes)
    tree = api.DeltaTree(codes, codebook=codebook)
    tree.write_files(d)
    nodes = os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n)
    assert os.path.getsize(nodes) == 60 * (n + 1)                      # QNode is 60 bytes, N+1 records (h:1484)
    assert np.array_equal(api.read_qnode_ids(nodes, n), tree.vec_id)
    rec = np.fromfile(nodes, dtype=np.uint8).reshape(n + 1, 60)
    assert np.array_equal(rec[:n, 33], tree.depth) and rec[0, 32] == 8
    assert np.array_equal(rec[0, 36:58:3], codes[tree.vec_id[0]])      # root diffs[m].to = root code (h:1437-1441)
    n_codes, payload = api.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    assert n_codes == n and np.array_equal(payload, tree.payload())
    edges = np.fromfile(os.path.join(d, "M8K256H1_Approx_Edges_N%d" % n), dtype=np.uint32)
    assert edges[0] == tree.vec_id[0] and len(edges) == 1 + 2 * (n - 1)


def test_numpy_encoder_reference_is_nearest_centroid():
    from deltapq_amd import synth
    from oracle import pq_encode_oracle
    v = synth.make_clustered_vectors(300, 128, seed=1, n_clusters=20)
    cb = synth.kmeans_codebook(v, 8, 16, iters=3, seed=2)
    codes = pq_encode_oracle.encode_pq(v, cb)
    d = ((v.reshape(300, 8, 1, 16).astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(-1)
    assert (codes == d.argmin(-1)).mean() > 0.99                       # fp32 vs fp64 may differ only on near ties


@pytest.mark.gpu
def test_gpu_pq_encoder_matches_fp32_reference(lib):
    from deltapq_amd import api, synth
    from oracle import pq_encode_oracle
    if api.device_count() < 1:
        pytest.fail("no GPU")
    v = synth.make_clustered_vectors(20000, 128, seed=3, n_clusters=400)
    cb = synth.kmeans_codebook(v, 8, 256, iters=4, seed=4)
    assert np.array_equal(api.encode_pq(v, cb), pq_encode_oracle.encode_pq(v, cb))     # bit-for-bit the same argmin
    cb16 = synth.kmeans_codebook(v, 16, 64, iters=2, seed=5)
    assert np.array_equal(api.encode_pq(v[:3000], cb16), pq_encode_oracle.encode_pq(v[:3000], cb16))


@pytest.mark.gpu
def test_end_to_end_vectors_to_query(lib, oracle):
    """learn -> encode (GPU) -> build tree (host) -> query (GPU): results, mapped back through
    vec_id, are the true PQ nearest neighbours of the raw codes."""
    from conftest import assert_parity, oracle_topk
    from deltapq_amd import api, synth
    if api.device_count() < 1:
        pytest.fail("no GPU")
    n, nq, k = 60000, 32, 20
    base = synth.make_clustered_vectors(n, 128, seed=11, n_clusters=1500)
    queries = synth.make_clustered_vectors(nq, 128, seed=12, n_clusters=1500)
    cb = synth.kmeans_codebook(base, 8, 256, iters=4, seed=13)
    codes = api.encode_pq(base, cb)
    tree = api.DeltaTree(codes, codebook=cb)
    payload = tree.payload()
    assert len(payload) < 0.8 * n * 8
    with api.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(cb)
        ids, dists = idx.query_batch(queries, k)
    assert_parity(ids, dists, oracle_topk(oracle, payload, n, cb, queries, k), n)
    pos = np.where(ids == n, n - 1, ids)                                # even-N quirk
    orig = tree.vec_id[pos]
    for i in range(nq):
        lut = oracle.build_lut(cb, queries[i])
        alld = sum(lut[m, codes[:, m]].astype(np.float64) for m in range(8)).astype(np.float32)
        assert np.array_equal(alld[orig[i]].view(np.uint32), dists[i].view(np.uint32))
        assert np.sort(alld)[k - 1] == dists[i][-1]                     # really the k best of the raw codes


@pytest.mark.parametrize("n,M,with_cb", [(1, 8, False), (2, 8, True), (3, 8, True), (700, 8, True), (6000, 8, True),
                                          (6000, 8, False), (2500, 16, True)])
def test_host_builder_matches_the_oracle_restatement(lib, n, M, with_cb):
    """The product's host builder against oracle/builder_oracle.py (an independent numpy restatement of
    h:445-627, h:1207-1313, h:1334-1487, h:1156-1183): same edges in the same order, same DFS layout, same stream."""
    from deltapq_amd import api, synth
    from oracle import builder_oracle
    codes = clustered_codes(n, M, seed=3 * n + M)
    cb = synth.make_codebook(M, 256, 4, seed=n) if with_cb else None
    ref = builder_oracle.build(codes, cb)
    t = api.DeltaTree(codes, codebook=cb)
    assert np.array_equal(t.edges, ref["edges"].reshape(-1, 2))
    assert np.array_equal(t.vec_id, ref["vec_id"]) and np.array_equal(t.depth, ref["depths"])
    assert np.array_equal(t.mask, ref["masks"]) and np.array_equal(t.deltas, ref["deltas"])
    assert np.array_equal(t.payload(), synth.encode_dtc(ref)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n,M", [(1, 8), (2, 8), (777, 8), (20000, 8), (8000, 16)])
def test_gpu_builder_matches_the_oracle_restatement(lib, n, M):
    """dpq_tree_build_gpu (edge search and tree layout on the device) against oracle/builder_oracle.py."""
    from deltapq_amd import api, synth
    from oracle import builder_oracle
    if api.device_count() < 1:
        pytest.fail("no GPU")
    codes = clustered_codes(n, M, seed=n + 11)
    cb = synth.make_codebook(M, 256, 4, seed=n)
    ref = builder_oracle.build(codes, cb)
    t = api.DeltaTree(codes, codebook=cb, device=0)
    assert np.array_equal(t.edges, ref["edges"].reshape(-1, 2))
    assert np.array_equal(t.vec_id, ref["vec_id"]) and np.array_equal(t.payload(), synth.encode_dtc(ref)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("what", [1, 2, 5, 30000, "two_values", "chain", "small_k"])
def test_gpu_layout_writes_the_same_artefact_files(lib, tmp_path, what):
    """The tree laid out on the GPU (adjacency, max_dist2p sibling order, DFS numbering, masks, changed bytes,
    sub-tree sizes, sqrt'ed max distances) against the host layout: the three artefact files byte for byte
    (the 60-byte QNode records carry every field of the layout).  `what`: a size of clustered codes, or one of the
    BUILD_CASES that come with a codebook."""
    import filecmp
    from deltapq_amd import api, synth
    if isinstance(what, str):
        codes, M, kw = build_case(what)
        assert M == 8 and kw.get("codebook") is not None
    else:
        n = what
        codes, kw = clustered_codes(n, 8, seed=n + 5), dict(codebook=synth.make_codebook(8, 256, 16, seed=n))
    dh, dd = tmp_path / "host", tmp_path / "dev"
    dh.mkdir()
    dd.mkdir()
    host, dev = api.DeltaTree(codes, **kw), api.DeltaTree(codes, device=0, **kw)
    host.write_files(str(dh))
    dev.write_files(str(dd))
    names = sorted(os.listdir(str(dh)))
    assert len(names) == 3 and names == sorted(os.listdir(str(dd)))
    for f in names:
        assert filecmp.cmp(str(dh / f), str(dd / f), shallow=False), f
    assert host.stats == dev.stats and np.array_equal(host.parent_pos, dev.parent_pos)


@pytest.mark.gpu
@pytest.mark.parametrize("n,M", [(1, 8), (2, 8), (777, 8), (50000, 8), (20000, 16)])
def test_gpu_edge_search_builds_the_identical_tree(lib, n, M):
    """SURVEY.md 8f row 1 on the GPU: the sort/group passes over every position subset run on the device
    (hipCUB stable radix sort + grouping kernels) and must reproduce the host builder exactly."""
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU")
    codes = clustered_codes(n, M, seed=n + 1)
    host = api.DeltaTree(codes)
    dev = api.DeltaTree(codes, device=0)
    assert np.array_equal(host.edges, dev.edges)
    assert np.array_equal(host.vec_id, dev.vec_id) and np.array_equal(host.payload(), dev.payload())
    assert host.stats == dev.stats


@pytest.mark.gpu
def test_gpu_edge_search_speed_and_structure_1m(lib):
    import time
    from deltapq_amd import api, synth
    n = 1_000_000
    tree = synth.synth_tree(n, 8, seed=102, mean_diffs=3.0)
    codes = synth.decode_tree_codes(tree)[np.random.default_rng(0).permutation(n)]
    t0 = time.time()
    dev = api.DeltaTree(codes, device=0)
    t_gpu = time.time() - t0
    assert dev.stats["n_diffs"] < 3.4 * n and dev.stats["max_depth"] <= 7
    assert np.array_equal(tree_decode(dev), codes[dev.vec_id])
    print("GPU-assisted build of 1M codes: %.2f s, %.2f diffs/node" % (t_gpu, dev.stats["n_diffs"] / n))
    assert t_gpu < 20


@pytest.mark.parametrize("seed", range(4))
def test_subset_prefilter_rule_keeps_every_member_of_a_group(seed):
    """find_edges_gpu's per-subset pre-filter (dpq_build_gpu.hip, keys_mark_kernel / hash_flag_kernel), restated in numpy: an
    open-addressing table of epoch | pair | fingerprint words, never cleared.  A node walks at most kProbes words from its
    slot: a word of an older epoch is free and is claimed; a word with the node's fingerprint gets its pair bit set; any
    other word is skipped.  A node is kept iff the word with its fingerprint carries the pair bit, or it found no word (then
    neither did any node with its key).  Whatever the order of arrival and whatever older epochs left in the table, every
    member of a group of >= 2 equal keys is kept, and a node alone under its key only by a fingerprint collision; the kept
    nodes in list order sort like the whole list does (the grouping returns on groups of one).  CPU only -- the kernels are
    checked by test_gpu_edge_search_builds_the_identical_tree."""
    rng = np.random.default_rng(seed)
    n, slots, probes = 5000, 1 << 13, 8                       # load ~0.6: probing and the not-placed case on purpose
    ep_of = np.zeros(slots, dtype=np.int64)                   # epoch 0 = never used
    pair = np.zeros(slots, dtype=bool)
    fp_of = np.zeros(slots, dtype=np.uint32)

    def h64(k):
        x = (k * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        x ^= x >> np.uint64(29)
        x = (x * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        return x ^ (x >> np.uint64(32))

    for epoch in (1, 2, 7):
        keys = rng.integers(0, 3000, size=n).astype(np.uint64)  # many groups of equal keys, many singletons
        with np.errstate(over="ignore"):
            h = h64(keys)
        fp = (h >> np.uint64(32)).astype(np.uint32)
        s0 = (h & np.uint64(slots - 1)).astype(np.int64)
        for i in rng.permutation(n):                            # CAS / OR semantics, arbitrary arrival order
            for p in range(probes):
                s = (s0[i] + p) & (slots - 1)
                if ep_of[s] != epoch:                           # free: claim
                    ep_of[s], pair[s], fp_of[s] = epoch, False, fp[i]
                    break
                if fp_of[s] == fp[i]:                           # this key is here already
                    pair[s] = True
                    break
        keep = np.ones(n, dtype=bool)                           # no word within `probes` steps: kept
        for i in range(n):
            for p in range(probes):
                s = (s0[i] + p) & (slots - 1)
                if ep_of[s] != epoch:
                    break
                if fp_of[s] == fp[i]:
                    keep[i] = pair[s]
                    break
        uniq, counts = np.unique(keys, return_counts=True)
        in_group = np.isin(keys, uniq[counts >= 2])
        assert keep[in_group].all()                             # no member of a clique is ever dropped
        assert (keep & ~in_group).sum() <= 0.02 * n + 8         # singles: fingerprint collisions / unplaced only
        order_all = np.argsort(keys, kind="stable")
        order_kept = np.flatnonzero(keep)[np.argsort(keys[keep], kind="stable")]
        grp = np.flatnonzero(in_group)
        assert np.array_equal(order_all[np.isin(order_all, grp)], order_kept[np.isin(order_kept, grp)])


# ---- the builder at its data-dependent paths: one table of named cases, compared three ways -------------------------
#
# find_edges_gpu / layout_tree_gpu (dpq_build_gpu.hip) choose their path by the data: how many nodes a subset's
# pre-filter keeps (one block up to kSmallMax = 2048, the radix-sort chain above), whether a key found a word in the pair
# table, which word of a 16-byte key differs, how tall the groups' members are.  Each case below is made to reach one
# of these; test_build_cases_reach_what_their_names_claim shows from the restatements that it does.

K_SMALL_MAX, K_PROBES = 2048, 8                      # dpq_build_gpu.hip: kSmallMax, kProbes
DPQ_ERR_FORMAT = -3


def _distinct_codes(rng, n, M):
    codes = np.unique(rng.integers(0, 256, size=(n + 64, M), dtype=np.uint8), axis=0)
    assert len(codes) >= n
    return codes[rng.permutation(len(codes))[:n]]


def _all_equal(M):
    return np.repeat(np.random.default_rng(20 + M).integers(0, 256, size=(1, M), dtype=np.uint8), 3000, axis=0), M, {}


def _all_ff_small(M):
    rng = np.random.default_rng(30 + M)
    # (at M = 16 the 500 other codes are clustered ones: 500 independent 16-byte codes stay unmerged through most of the
    # 2^16 position subsets, which costs the restatement ten seconds and shows nothing more)
    others = _distinct_codes(rng, 500, M) if M == 8 else clustered_codes(500, M, seed=33)
    assert not (others == 0xFF).all(1).any()
    codes = np.concatenate((np.full((1500, M), 0xFF, dtype=np.uint8), others))
    return codes[rng.permutation(len(codes))], M, {}


def _pairs(n_pairs):
    rng = np.random.default_rng(n_pairs)
    d = _distinct_codes(rng, n_pairs + 3000, 8)
    codes = np.concatenate((d[:n_pairs], d))
    return codes[rng.permutation(len(codes))], 8, {}


def max_agreement(codes):
    """The largest number of positions on which two different rows agree, and the rows that reach it."""
    best, rows = -1, []
    for lo in range(0, len(codes), 500):
        agree = (codes[lo:lo + 500, None, :] == codes[None, :, :]).sum(-1)
        agree[np.arange(len(agree)), lo + np.arange(len(agree))] = -1
        top = int(agree.max())
        if top > best:
            best, rows = top, []
        if top == best:
            rows += (lo + np.flatnonzero((agree == top).any(1))).tolist()
    return best, rows


def _all_distinct_far():
    rng = np.random.default_rng(40)
    codes = rng.integers(0, 256, size=(4000, 8), dtype=np.uint8)
    while True:
        top, rows = max_agreement(codes)
        if top <= 2:
            return codes, 8, {}
        codes[rows[1::2]] = rng.integers(0, 256, size=(len(rows[1::2]), 8), dtype=np.uint8)   # redraw one of each pair


def _chain(folds, with_cb):
    from deltapq_amd import synth
    rng = np.random.default_rng(5)
    codes = np.zeros((2000, 8), dtype=np.uint8)
    codes[0] = rng.integers(0, 256, size=8)
    for i in range(1, len(codes)):                   # code i differs from code i - 1 in position (i - 1) % 8 alone
        codes[i] = codes[i - 1]
        p = (i - 1) % 8
        codes[i, p] = (int(codes[i, p]) + int(rng.integers(1, 256))) % 256
    kw = dict(max_height_folds=folds)
    if with_cb:
        kw["codebook"] = synth.make_codebook(8, 256, 4, seed=50)
    return codes, 8, kw


def _two_values():
    from deltapq_amd import synth
    rng = np.random.default_rng(60)
    return rng.choice(np.array([0, 255], dtype=np.uint8), size=(5000, 8)), 8, dict(codebook=synth.make_codebook(8, 256, 4, seed=61))


def _one_word_m16(varying_hi):
    rng = np.random.default_rng(70 + varying_hi)
    codes = np.repeat(rng.integers(1, 256, size=(1, 16), dtype=np.uint8), 2500, axis=0)
    half = slice(8, 16) if varying_hi else slice(0, 8)
    codes[:, half] = clustered_codes(2500, 8, seed=71 + varying_hi)
    return codes, 16, {}


def _small_k():
    from deltapq_amd import synth
    return clustered_codes(3000, 8, seed=80) & 15, 8, dict(K=16, codebook=synth.make_codebook(8, 16, 4, seed=81))


def key_hash(lo, hi=0):
    """key_hash of dpq_build_gpu.hip, restated: the pair table's slot is the low bits, the fingerprint the high word."""
    m64 = (1 << 64) - 1
    lo = np.asarray(lo, dtype=np.uint64)
    h = lo * np.uint64(0x9E3779B97F4A7C15)
    h = h ^ np.uint64((((hi + 0x7F4A7C159E3779B9) & m64) * 0xC2B2AE3D27D4EB4F) & m64)
    h = h ^ (h >> np.uint64(29))
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    return h ^ (h >> np.uint64(32))


def probe_window_codes():
    """14 distinct 8-byte codes whose full-mask keys start their probe sequences inside ONE window of four consecutive
    slots of a 2^16-slot table (what n <= 16384 gets)."""
    rng = np.random.default_rng(90)
    draws = _distinct_codes(rng, 400000, 8)
    slot = (key_hash(np.ascontiguousarray(draws).view("<u8").ravel()) & np.uint64(0xFFFF)).astype(np.int64)
    per_slot = np.bincount(slot, minlength=1 << 16)
    window = per_slot[:-3] + per_slot[1:-2] + per_slot[2:-1] + per_slot[3:]
    s = int(window.argmax())
    assert window[s] >= 14
    return draws[np.flatnonzero((slot >= s) & (slot < s + 4))[:14]]


def _probe_run(n_dups):
    """The pre-filter's `found no word` branch.  The hash is restated from the kernel ON PURPOSE: 14 keys whose probe
    sequences start within four consecutive slots reach 4 + kProbes - 1 = 11 words between them, so whatever the order
    of arrival at least three of them find no word within kProbes steps; such a node is kept, and its duplicate has
    to be merged under it at diff 0 all the same.  Should the hash change, the case stops reaching the branch and
    test_build_cases_reach_what_their_names_claim says so."""
    rng = np.random.default_rng(91)
    w = probe_window_codes()
    codes = np.concatenate((w, w[:n_dups], _distinct_codes(rng, 4000 - 14 - n_dups, 8)))
    return codes[rng.permutation(len(codes))], 8, {}


def _hypercube_folds2():
    """Case H of test_hand_derived_builder.py (all 256 codes over two values per position, in counting order) with
    max_height_folds = 2: nothing is frozen below height 14, the tree is the binomial tree B8, nine levels deep, and
    the 3-bit depth field of the stream cannot hold that.  The host refuses (DPQ_ERR_FORMAT); so must the GPU."""
    import itertools
    return np.array(list(itertools.product(*[(1, 2)] * 8)), dtype=np.uint8), 8, dict(max_height_folds=2)


def _tiny_m16(n):
    return clustered_codes(n, 16, seed=100 + n), 16, {}


BUILD_CASES = {
    "all_equal_m8": lambda: _all_equal(8), "all_equal_m16": lambda: _all_equal(16),
    "all_ff_m8_small": lambda: _all_ff_small(8), "all_ff_m16_small": lambda: _all_ff_small(16),
    "pairs_2046": lambda: _pairs(1023), "pairs_2048": lambda: _pairs(1024), "pairs_2050": lambda: _pairs(1025),
    "all_distinct_far": _all_distinct_far,
    "chain": lambda: _chain(1, True), "chain_folds2": lambda: _chain(2, False),
    "two_values": _two_values,
    "hi_word_only_m16": lambda: _one_word_m16(True), "lo_word_only_m16": lambda: _one_word_m16(False),
    "small_k": _small_k,
    "probe_run": lambda: _probe_run(6), "probe_run_all": lambda: _probe_run(14),
    "hypercube_folds2": _hypercube_folds2,
    "m16_n1": lambda: _tiny_m16(1), "m16_n2": lambda: _tiny_m16(2), "m16_n3": lambda: _tiny_m16(3),
}
REFUSED = {"hypercube_folds2": DPQ_ERR_FORMAT}       # what the host answers; the GPU has to answer the same
_built, _refs = {}, {}


def build_case(name):
    if name not in _built:
        codes, M, kw = BUILD_CASES[name]()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.shape[1] == M
        codes.setflags(write=False)
        _built[name] = (codes, M, kw)
    return _built[name]


def restated(name):
    """oracle/builder_oracle.py on a case; computed once, shared, left unchanged."""
    from oracle import builder_oracle
    if name not in _refs:
        codes, _, kw = build_case(name)
        _refs[name] = builder_oracle.build(codes, kw.get("codebook"), kw.get("max_height_folds", 1))
    return _refs[name]


def assert_same_tree(a, b):
    for field in ("edges", "vec_id", "parent_pos", "depth", "mask", "deltas", "root"):
        assert np.array_equal(getattr(a, field), getattr(b, field)), field
    assert np.array_equal(a.payload(), b.payload())
    assert a.stats == b.stats


@pytest.mark.parametrize("name", sorted(BUILD_CASES))
def test_host_builder_on_the_build_cases(lib, name):
    """The host build against oracle/builder_oracle.py on every case of the table, and lossless.  (The restatement
    takes a few seconds at most on each: n <= 6000 at M = 8, n <= 3000 at M = 16 where everything merges early.)"""
    from deltapq_amd import _lib, api, synth
    codes, M, kw = build_case(name)
    assert len(codes) <= (6000 if M == 8 else 3000)
    ref = restated(name)
    if name in REFUSED:
        assert int(ref["depths"].max()) >= (8 if M <= 8 else 16)      # the restatement has no depth field to overflow
        with pytest.raises(_lib.DpqError) as e:
            api.DeltaTree(codes, **kw)
        assert e.value.status == REFUSED[name]
        return
    t = api.DeltaTree(codes, **kw)
    assert np.array_equal(t.edges, ref["edges"].reshape(-1, 2))
    assert np.array_equal(t.vec_id, ref["vec_id"]) and np.array_equal(t.depth, ref["depths"])
    assert np.array_equal(t.parent_pos, ref["parent_pos"])
    assert np.array_equal(t.mask, ref["masks"]) and np.array_equal(t.deltas, ref["deltas"])
    assert np.array_equal(t.payload(), synth.encode_dtc(ref)[0])
    assert np.array_equal(tree_decode(t), codes[t.vec_id])
    assert t.stats["max_depth"] == int(ref["depths"].max())


def test_build_cases_reach_what_their_names_claim():
    """Non-vacuity.  The evidence is the data and the restatements' output, never the GPU's."""
    from oracle import builder_oracle

    def multiplicity(codes):
        return np.unique(codes, axis=0, return_counts=True)[1]

    for M in (8, 16):
        codes, _, _ = build_case("all_equal_m%d" % M)
        assert len(codes) > K_SMALL_MAX and multiplicity(codes).tolist() == [len(codes)]     # one group, the long path
        assert (restated("all_equal_m%d" % M)["masks"] == 0).all()
        codes, _, _ = build_case("all_ff_m%d_small" % M)
        ff = (codes == 0xFF).all(1)
        # real keys equal to the bitonic sort's padding key, and padding present: 1024 < n_keep <= 2000 < P = 2048
        assert ff.sum() == 1500 and len(codes) == 2000 < K_SMALL_MAX
        assert M == 16 or multiplicity(codes[~ff]).max() == 1
    for kept in (2046, 2048, 2050):                  # below the switch with padding, at it, above it
        codes, _, _ = build_case("pairs_%d" % kept)
        mult = multiplicity(codes)
        assert (mult == 2).sum() * 2 == kept and (mult > 2).sum() == 0 and (mult == 1).sum() == 3000
        assert (kept <= K_SMALL_MAX) == (kept != 2050)
        assert (restated("pairs_%d" % kept)["masks"][1:] == 0).sum() == kept // 2             # merged at diff 0, all of them

    codes, _, _ = build_case("all_distinct_far")
    assert max_agreement(codes)[0] == 2              # nothing can merge before diff 6: 93 subsets keep fewer than two
    fin, edges = builder_oracle.find_edges(codes)
    assert min((codes[p] != codes[c]).sum() for p, c in edges) >= 6

    for name, folds in (("chain", 1), ("chain_folds2", 2)):
        codes, _, kw = build_case(name)
        assert kw["max_height_folds"] == folds
        step = codes[1:] != codes[:-1]
        assert (step.sum(1) == 1).all() and np.array_equal(step.argmax(1), np.arange(len(codes) - 1) % 8)
        fin, _ = builder_oracle.find_edges(codes, folds)
        # folds 1: the cap M - 2 = 6 is reached (finalists beyond the one node left over), the tree is as deep as the
        # cap lets a merge tree be; folds 2: the cap is 14 and nothing is frozen
        assert (len(fin) >= 2) == (folds == 1)
        assert int(restated(name)["depths"].max()) == 6
    assert int(restated("hypercube_folds2")["depths"].max()) == 8

    codes, _, kw = build_case("two_values")
    assert set(np.unique(codes)) == {0, 255} and kw["codebook"].shape == (8, 256, 4)
    mult = multiplicity(codes)
    assert len(mult) == 256 and mult.min() >= 5      # every code of the cube, each many times: long sibling lists
    ref = restated("two_values")
    n_children = np.bincount(ref["parent_pos"][1:].astype(np.int64), minlength=len(codes))
    assert n_children.max() >= 10
    # equal max_dist2p among siblings (the duplicates: distance 0 to the parent): their order is the edge order
    dup_kids = np.bincount(ref["parent_pos"][1:].astype(np.int64)[ref["masks"][1:] == 0], minlength=len(codes))
    assert dup_kids.max() >= 5

    for name, same in (("hi_word_only_m16", slice(0, 8)), ("lo_word_only_m16", slice(8, 16))):
        codes, M, _ = build_case(name)
        assert M == 16 and (codes[:, same] == codes[0, same]).all() and (codes[0, same] != 0).all()
        other = slice(8, 16) if same.start == 0 else slice(0, 8)
        assert len(np.unique(codes[:, other], axis=0)) > 1000

    codes, _, kw = build_case("small_k")
    assert codes.max() == 15 and kw["K"] == 16 and kw["codebook"].shape == (8, 16, 4)

    w = probe_window_codes()
    h = key_hash(np.ascontiguousarray(w).view("<u8").ravel())
    slot, fp = (h & np.uint64(0xFFFF)).astype(np.int64), (h >> np.uint64(32))
    assert len(np.unique(w, axis=0)) == 14 and len(np.unique(fp)) == 14
    assert slot.max() - slot.min() <= 3              # 14 keys, 3 + kProbes = 11 words within reach: three find none
    assert 14 - (slot.max() - slot.min() + K_PROBES) >= 3
    for name, n_dups in (("probe_run", 6), ("probe_run_all", 14)):
        codes, _, _ = build_case(name)
        assert len(codes) == 4000 and 4 * len(codes) <= 1 << 16                # the table has 2^16 slots
        mult = multiplicity(codes)
        assert (mult == 2).sum() == n_dups and mult.max() == 2
        in_w = (codes[:, None, :] == w[None]).all(-1).any(1)
        assert in_w.sum() == 14 + n_dups
        assert (restated(name)["masks"][1:] == 0).sum() == n_dups               # every duplicate merged at diff 0

    for n in (1, 2, 3):
        codes, M, _ = build_case("m16_n%d" % n)
        assert codes.shape == (n, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BUILD_CASES))
def test_gpu_builder_on_the_build_cases(lib, name):
    """The GPU build (edge search and layout on the device) against the host build on every case of the table: edges,
    DFS order, parents, depths, masks, changed bytes, the stream and the statistics; and lossless."""
    from deltapq_amd import _lib, api
    if api.device_count() < 1:
        pytest.fail("no GPU")
    codes, M, kw = build_case(name)
    if name in REFUSED:
        with pytest.raises(_lib.DpqError) as host:
            api.DeltaTree(codes, **kw)
        with pytest.raises(_lib.DpqError) as dev:
            api.DeltaTree(codes, device=0, **kw)
        assert dev.value.status == host.value.status == REFUSED[name]
        return
    host, dev = api.DeltaTree(codes, **kw), api.DeltaTree(codes, device=0, **kw)
    assert_same_tree(host, dev)
    assert np.array_equal(tree_decode(dev), codes[dev.vec_id])
