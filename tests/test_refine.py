"""Residual re-ranking (dpq_refine_*, dpq_residuals, dpq_query_batch_refined): a second PQ level over the residuals of an
index's nodes re-ranks a PQ shortlist.  Every GPU comparison is exact -- code bytes equal, floats bit-equal -- against
tests/_refine_restatement.py, the rules of include/deltapq_amd.h in numpy; the restatement itself is pinned by
hand-derived cases, and the GPU answers are cross-checked against the merged exact re-ranker over the x rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _kmeans_restatement as KM
import _refine_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
ERR_ARG, ERR_NO_DEVICE, ERR_STATE, ERR_TOPK = -1, -4, -7, -8
REFINE_SYMBOLS = ("dpq_residuals", "dpq_refine_create", "dpq_refine_free", "dpq_refine_get", "dpq_refine_build",
                  "dpq_refine_reconstruct", "dpq_refine_rerank", "dpq_refine_rerank_device", "dpq_query_batch_refined")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """(ids, dists) pairs equal: ids exactly, distances to the bit."""
    return np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


# ---- CPU ------------------------------------------------------------------------------------------------------------

def one_node_level(a0, b0):
    """One node, M = 8, Ds = 1, M2 = 8: a = (a0, 0, ..), b = (b0, 0, ..)."""
    cb1 = np.zeros((8, 2, 1), dtype=np.float32)
    cb2 = np.zeros((8, 2, 1), dtype=np.float32)
    cb1[0, 1, 0], cb2[0, 1, 0] = a0, b0
    c = np.zeros((1, 8), dtype=np.uint8)
    c[0, 0] = 1
    return R.reconstruct(cb1, c, cb2, c)


def test_restatement_hand_derived_half_ulp_is_rounded_away():
    """a[0] = 1, b[0] = 2^-24, q[0] = 1: x[0] = fl(1 + 2^-24) = 1 (a tie, to even), so the distance is +0.0.  Evaluating
    (q - a) - b instead gives -2^-24 and a distance of 2^-48 = 0x27800000."""
    x = one_node_level(1.0, 2.0 ** -24)
    assert bits(x)[0, 0] == 0x3F800000 and not bits(x)[0, 1:].any()
    q = np.zeros((1, 8), dtype=np.float32)
    q[0, 0] = 1.0
    ids, d = R.rerank(x, q, np.array([[0]]), 1, n_total=1)
    assert ids[0, 0] == 0 and bits(d)[0, 0] == 0x00000000
    other = np.float32((np.float32(1.0) - np.float32(1.0)) - np.float32(2.0 ** -24))
    assert bits(np.float32(other * other)) == 0x27800000


def test_restatement_hand_derived_tie_to_even_upwards():
    """a[0] = 1 + 2^-23 (odd mantissa), b[0] = 2^-24 (half an ulp): x[0] = fl(a + b) = 1 + 2^-22 (the tie goes to the even
    neighbour, upwards); with q[0] = 1, t = 2^-22 and the distance is 2^-44 = 0x29800000.  An fp64 (or fused) evaluation
    keeps x = 1 + 1.5 * 2^-23 and answers 2.25 * 2^-46 instead."""
    a0 = np.float32(1.0 + 2.0 ** -23)
    x = one_node_level(a0, 2.0 ** -24)
    assert bits(x)[0, 0] == 0x3F800002
    q = np.zeros((1, 8), dtype=np.float32)
    q[0, 0] = 1.0
    _, d = R.rerank(x, q, np.array([[0, -1, 0]]), 2, n_total=1)
    assert bits(d)[0, 0] == 0x29800000 and np.isinf(d[0, 1])
    wide = (float(a0) + 2.0 ** -24 - 1.0) ** 2
    assert bits(np.float32(wide)) != 0x29800000 and np.float32(wide) == np.float32(2.25 * 2.0 ** -46)


def test_restatement_ids_follow_the_lookup_rules():
    assert R.local_of([0, 9, 10, 8], 0, 10, 10).tolist() == [0, -1, 9, 8]          # even N: N names the last node
    assert R.local_of([0, 10, 11], 0, 11, 11).tolist() == [0, 10, -1]
    assert R.local_of([5, 4, 9, 10], 5, 10, 10).tolist() == [0, -1, -1, 4]         # a shard that ends an even index
    assert R.local_of([9, 10], 0, 10, 10, even_rule=False).tolist() == [9, -1]     # a plain handle
    assert R.shape_ok(40, 3, 7, 14) and not R.shape_ok(40, 16, 16, 3) and R.shape_ok(112, 16, 16, 7)
    assert not R.shape_ok(8, 16, 16, 1) and not R.shape_ok(40, 3, 7, 13) and not R.shape_ok(40, 65, 2, 1)
    assert R.sample_positions(10, 4) == [0, 2, 5, 7]


def test_restatement_level_is_not_vacuous():
    """On clustered vectors the two-level reconstruction is strictly closer to the vectors than level 1 alone."""
    from deltapq_amd import synth
    from oracle import pq_encode_oracle as E
    v = synth.make_clustered_vectors(4000, 32, seed=3, n_clusters=50)
    cb1, _ = KM.train(v, 8, 16, max_iters=6, seed=1)
    c1 = E.encode_pq(v, cb1)
    res = R.residuals(v, cb1, c1)
    cb2, _ = KM.train(res, 8, 16, max_iters=6, seed=2)
    c2 = R.encode2(res, cb2)
    a = R.level1(cb1, c1).astype(np.float64)
    x = R.reconstruct(cb1, c1, cb2, c2).astype(np.float64)
    e1, e2 = ((a - v) ** 2).sum(), ((x - v) ** 2).sum()
    print("summed squared error: level 1 %.6g, two levels %.6g" % (e1, e2))
    assert e2 < e1


def test_refine_symbols_declared_exported_and_bound(lib):
    from deltapq_amd import _lib, api
    names = {name for name, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in REFINE_SYMBOLS:
        assert name in names and name + "(" in header and hasattr(raw, name), name
    assert "dpq_refine_opts" in header and ctypes.sizeof(_lib.RefineOpts) == 2 * 4 + 8 + 4 * 4 + 8
    for attr in ("build", "from_arrays", "arrays", "residuals", "reconstruct", "rerank", "rerank_torch",
                 "query_batch_refined", "close", "__enter__", "__exit__"):
        assert hasattr(api.RefineLevel, attr), attr


def test_refine_argument_errors_come_before_the_device(lib):
    """Everything that can be judged without reading a handle is DPQ_ERR_ARG with or without a GPU.  (The rules that need
    the handle's D1 -- Ds2 against ceil(D1 / M2), the empty sub-space, D against Ds -- are in the GPU tests: no handle
    exists without a device.)"""
    from deltapq_amd import _lib
    buf = np.zeros(1 << 12, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: the argument checks come first
    out = ctypes.c_void_p()
    # NULLs
    assert lib.dpq_residuals(None, p, 1, p, 8, p) == ERR_ARG
    assert lib.dpq_residuals(fake, None, 1, p, 8, p) == ERR_ARG
    assert lib.dpq_residuals(fake, p, 1, None, 8, p) == ERR_ARG
    assert lib.dpq_residuals(fake, p, 1, p, 8, None) == ERR_ARG
    assert lib.dpq_residuals(fake, p, -1, p, 8, p) == ERR_ARG
    assert lib.dpq_residuals(fake, p, 1, p, 0, p) == ERR_ARG                          # D < 1 matches no Ds
    assert lib.dpq_refine_create(None, p, 8, 16, 1, p, 1, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_create(fake, None, 8, 16, 1, p, 1, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_create(fake, p, 8, 16, 1, None, 1, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_create(fake, p, 8, 16, 1, p, 1, None) == ERR_ARG
    assert lib.dpq_refine_get(None, None, None, None, None, None, None) == ERR_ARG
    assert lib.dpq_refine_build(None, p, 1, 8, None, None, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_build(fake, None, 1, 8, None, None, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_build(fake, p, 1, 8, None, None, None) == ERR_ARG
    assert lib.dpq_refine_build(fake, p, 0, 8, None, None, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_build(fake, p, 1, 0, None, None, ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_reconstruct(None, p, 1, p) == ERR_ARG
    assert lib.dpq_refine_reconstruct(fake, None, 1, p) == ERR_ARG
    assert lib.dpq_refine_reconstruct(fake, p, 1, None) == ERR_ARG
    lib.dpq_refine_free(None)                                                         # nothing happens
    # the shape of a level
    for M2, K2, Ds2 in ((0, 16, 1), (65, 16, 1), (-1, 16, 1), (8, 1, 1), (8, 257, 1), (8, 0, 1), (8, 16, 0), (8, 16, -3)):
        assert lib.dpq_refine_create(fake, p, M2, K2, Ds2, p, 1, ctypes.byref(out)) == ERR_ARG, (M2, K2, Ds2)
    assert lib.dpq_refine_create(fake, p, 8, 16, 1, p, 0, ctypes.byref(out)) == ERR_ARG
    for M2, K2 in ((65, 0), (-1, 0), (0, 1), (0, 257), (0, -2)):
        o = _lib.RefineOpts(M2=M2, K2=K2)
        assert lib.dpq_refine_build(fake, p, 1, 8, None, o, ctypes.byref(out)) == ERR_ARG, (M2, K2)
    assert lib.dpq_refine_build(fake, p, 1, 8, None, _lib.RefineOpts(train_n=-1), ctypes.byref(out)) == ERR_ARG
    assert lib.dpq_refine_build(fake, p, 1, 8, None, _lib.RefineOpts(max_iters=65), ctypes.byref(out)) == ERR_ARG
    # top_k / n_cand
    for fn in (lambda *a: lib.dpq_refine_rerank(*a), lambda *a: lib.dpq_refine_rerank_device(*a, None)):
        assert fn(None, p, 1, p, 4, 2, p, p) == ERR_ARG
        assert fn(fake, None, 1, p, 4, 2, p, p) == ERR_ARG
        assert fn(fake, p, 1, None, 4, 2, p, p) == ERR_ARG
        assert fn(fake, p, 1, p, 4, 2, None, p) == ERR_ARG
        assert fn(fake, p, 1, p, 4, 2, p, None) == ERR_ARG
        assert fn(fake, p, -1, p, 4, 2, p, p) == ERR_ARG
        for n_cand, top_k in ((4, 0), (4, 5), (0, 0), (16385, 1), (16385, 16385), (4, -1)):
            assert fn(fake, p, 1, p, n_cand, top_k, p, p) == ERR_ARG, (n_cand, top_k)
    assert lib.dpq_query_batch_refined(None, fake, None, p, 1, 4, 2, p, p) == ERR_ARG
    assert lib.dpq_query_batch_refined(fake, None, None, p, 1, 4, 2, p, p) == ERR_ARG
    assert lib.dpq_query_batch_refined(fake, fake, None, None, 1, 4, 2, p, p) == ERR_ARG
    assert lib.dpq_query_batch_refined(fake, fake, None, p, 1, 4, 2, None, p) == ERR_ARG
    assert lib.dpq_query_batch_refined(fake, fake, None, p, 1, 4, 5, p, p) == ERR_ARG
    assert lib.dpq_query_batch_refined(fake, fake, None, p, 1, 16385, 5, p, p) == ERR_ARG
    assert b"n_cand" in lib.dpq_last_error()
    if lib.dpq_device_count() == 0:   # ... and with acceptable arguments the missing device is what is reported
        assert lib.dpq_refine_create(fake, p, 8, 16, 1, p, 1, ctypes.byref(out)) == ERR_NO_DEVICE
        assert lib.dpq_refine_rerank(fake, p, 1, p, 4, 2, p, p) == ERR_NO_DEVICE
        assert lib.dpq_residuals(fake, p, 1, p, 8, p) == ERR_NO_DEVICE


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def raises(gpu, status, fn, *args, **kw):
    with pytest.raises(gpu.DpqError) as e:
        fn(*args, **kw)
    assert e.value.status == status, e.value


def make_tree(n, M, seed, dup=True):
    from deltapq_amd import synth
    tree = synth.synth_tree(n, M, seed=seed, mean_diffs=(0.35 if M == 8 else 0.7) if dup else (3.0 if M == 8 else 5.0))
    payload, _ = synth.encode_dtc(tree)
    return payload, synth.decode_tree_codes(tree)


def make_vectors(cb1, codes1, D, seed, scale=6.0):
    """Raw vectors [n][D] near their level-1 reconstruction, so that residuals are small and structured."""
    rng = np.random.default_rng(seed)
    a = R.level1(cb1, codes1)[:, :D]
    return (a + rng.normal(0.0, scale, size=a.shape)).astype(np.float32)


def make_level(cb1, codes1, vectors, M2, K2, seed):
    """(codewords2, codes2, residual rows): a random codebook around the residuals' spread, codes by the restatement;
    nodes with equal level-1 codes are given equal level-2 codes too, pairwise, so that equal distances occur."""
    rng = np.random.default_rng(seed)
    D1 = cb1.shape[0] * cb1.shape[2]
    Ds2 = -(-D1 // M2)
    res = R.residuals(vectors, cb1, codes1)
    cb2 = rng.normal(0.0, 5.0, size=(M2, K2, Ds2)).astype(np.float32)
    codes2 = R.encode2(res, cb2)
    _, first, inv = np.unique(codes1, axis=0, return_index=True, return_inverse=True)
    twins = first[inv.reshape(-1)]
    sel = (np.arange(len(codes1)) % 2 == 0)
    codes2[sel] = codes2[twins[sel]]
    return cb2, codes2, res


def reportable(n_lo, n_hi, n_total, even_rule=True):
    ids = np.arange(n_lo, n_hi, dtype=np.int64)
    if even_rule and n_total % 2 == 0:
        ids[ids == n_total - 1] = n_total
    return ids.astype(np.int32)


def make_candidates(ids, nq, n_cand, seed):
    """[nq][n_cand] over the handle's reportable ids: repeats, padding, the last node twice, one nearly empty row."""
    rng = np.random.default_rng(seed)
    c = ids[rng.integers(0, len(ids), size=(nq, n_cand))].astype(np.int32)
    c[rng.random(size=c.shape) < 0.15] = -1
    c[0, 0] = ids[-1]
    c[0, -1] = ids[-1]
    if n_cand > 2:
        c[-1, 2:] = -1                    # fewer valid candidates than top_k = n_cand
        c[-1, 1] = c[-1, 0]               # ... one of them named twice
    return c


# n, chunks_per_segment, M, Ds, M2, K2, n_cand, nq
SHAPES = [
    (1, 1, 8, 1, 8, 256, 1, 1),
    (2, 2, 8, 3, 3, 7, 63, 3),
    (65, 1, 8, 4, 8, 256, 64, 70),
    (129, 2, 8, 5, 3, 7, 65, 3),
    (1000, 1, 8, 5, 1, 2, 255, 1),
    (1001, 2, 8, 16, 8, 256, 256, 3),
    (1000, 2, 16, 7, 16, 16, 257, 3),
    (1001, 1, 8, 16, 16, 16, 1000, 3),
    (1000, 1, 16, 7, 3, 7, 1000, 70),
    (129, 2, 8, 16, 1, 2, 16384, 2),
    (1000, 2, 8, 3, 8, 256, 255, 70),
    (2, 1, 8, 1, 1, 2, 64, 3),
    (65, 2, 8, 4, 8, 256, 600, 3),      # 1024 key slots in four workgroups, the last one all padding
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,cps,M,Ds,M2,K2,n_cand,nq", SHAPES)
def test_residuals_reconstruct_rerank_bit_for_bit(gpu, n, cps, M, Ds, M2, K2, n_cand, nq):
    import torch
    from deltapq_amd import synth
    D1 = M * Ds
    D = D1 - 1 if D1 >= 24 else D1
    seed = n * 131 + M * 17 + Ds
    payload, codes1 = make_tree(n, M, seed)
    cb1 = synth.make_codebook(M, 256, Ds, seed=seed + 1)
    v = make_vectors(cb1, codes1, D, seed + 2)
    cb2, codes2, res = make_level(cb1, codes1, v, M2, K2, seed + 3)
    xrows = R.reconstruct(cb1, codes1, cb2, codes2)
    ids = reportable(0, n, n)
    rng = np.random.default_rng(seed + 4)
    queries = (xrows[rng.integers(0, n, size=nq)] + rng.normal(0.0, 8.0, size=(nq, D1))).astype(np.float32)
    cand = make_candidates(ids, nq, n_cand, seed + 5)
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256, chunks_per_segment=cps) as idx:
        assert idx.info()["chunks_per_segment"] == cps
        raises(gpu, ERR_STATE, gpu.RefineLevel.from_arrays, idx, cb2, codes2)             # before the codebook
        raises(gpu, ERR_STATE, gpu.RefineLevel.residuals, idx, ids, v)
        idx.set_codebook(cb1)
        # residuals: every node, then a request with padding and repeats
        assert np.array_equal(bits(gpu.RefineLevel.residuals(idx, ids, v)), bits(res))
        sel = rng.integers(0, n, size=50)
        req = ids[sel].copy()
        req[::7] = -1
        got = gpu.RefineLevel.residuals(idx, req, v[sel])
        assert (bits(got[req < 0]) == R.NAN_BITS).all() and np.array_equal(bits(got[req >= 0]), bits(res[sel][req >= 0]))
        if D1 >= 24:
            raises(gpu, ERR_ARG, gpu.RefineLevel.residuals, idx, ids, v[:, :M * (Ds - 1)])   # ceil(D / M) != Ds
        if n % 2 == 0:
            raises(gpu, ERR_ARG, gpu.RefineLevel.residuals, idx, [n - 1], v[:1])
        raises(gpu, ERR_ARG, gpu.RefineLevel.residuals, idx, [n + 1], v[:1])
        with gpu.RefineLevel.from_arrays(idx, cb2, codes2) as lvl:
            assert (lvl.M2, lvl.K2, lvl.Ds2, lvl.n_local, lvl.D1) == (M2, K2, cb2.shape[2], n, D1)
            gcw, gc = lvl.arrays()
            assert np.array_equal(bits(gcw), bits(cb2)) and np.array_equal(gc, codes2)
            # reconstruction
            assert np.array_equal(bits(lvl.reconstruct(ids)), bits(xrows))
            got = lvl.reconstruct(req)
            assert (bits(got[req < 0]) == R.NAN_BITS).all() and np.array_equal(bits(got[req >= 0]), bits(xrows[sel][req >= 0]))
            assert lvl.reconstruct([]).shape == (0, D1)
            if n % 2 == 0:
                assert np.array_equal(bits(lvl.reconstruct([n])), bits(xrows[-1:]))       # id n names the last node
                raises(gpu, ERR_ARG, lvl.reconstruct, [n - 1])
            # re-ranking: host form, then the device form on a stream of its own into pre-filled outputs
            tq, tc = torch.from_numpy(queries).cuda(), torch.from_numpy(cand).cuda()
            stream = torch.cuda.Stream()
            for top_k in sorted({1, n_cand}):
                want = R.rerank(xrows, queries, cand, top_k, n_total=n)
                if top_k == n_cand and n_cand > 2:
                    assert want[0][-1, 1] == -1 and np.isinf(want[1][-1, 1])             # a padded row is in the case
                assert same(lvl.rerank(queries, cand, top_k), want), top_k
                oi = torch.full((nq, top_k), 77, dtype=torch.int32, device="cuda")
                od = torch.full((nq, top_k), -3.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    ri, rd = lvl.rerank_torch(tq, tc, top_k, out_ids=oi, out_dists=od)
                assert ri is oi and rd is od and same((oi.cpu().numpy(), od.cpu().numpy()), want), top_k
            # equal distances are ordered by id
            both = R.rerank(xrows, queries, cand, n_cand, n_total=n)
            if n >= 1000 and nq >= 3:
                d = both[1][:-1]
                assert ((d[:, 1:] == d[:, :-1]) & np.isfinite(d[:, 1:])).any(), "the case holds no equal distances"
            # a candidate that names no node: the host form before any device work, the device form by its flag
            bad = cand.copy()
            bad[nq - 1, n_cand // 2] = n + 1 if n % 2 else n - 1
            raises(gpu, ERR_ARG, lvl.rerank, queries, bad, 1)
            raises(gpu, ERR_ARG, lvl.rerank_torch, tq, torch.from_numpy(bad).cuda(), 1)
            assert same(lvl.rerank(queries, cand, 1), R.rerank(xrows, queries, cand, 1, n_total=n))   # and works on
            # the merged exact re-ranker over the x rows gives the same answer (candidates that need no renaming)
            plain = np.where(cand == n, -1, cand) if n % 2 == 0 else cand
            with gpu.FlatIndex(xrows) as flat:
                flat.set_id_map(np.arange(n, dtype=np.uint32))
                k = min(n_cand, 10)
                assert same(lvl.rerank(queries, plain, k), flat.rerank(queries, plain, k))


@pytest.mark.gpu
def test_level_shapes_the_contract_refuses(gpu):
    from deltapq_amd import synth
    n = 129
    payload, codes1 = make_tree(n, 8, 5)
    cb1 = synth.make_codebook(8, 256, 5, seed=1)          # D1 = 40
    v = make_vectors(cb1, codes1, 39, 2)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(cb1)
        z = np.zeros((n, 64), dtype=np.uint8)
        for M2, K2, Ds2 in ((16, 16, 3),      # (M2 - 1) * Ds2 = 45 >= 40: sub-spaces without a real dimension
                            (3, 7, 13), (3, 7, 15), (8, 256, 4), (40, 2, 2), (64, 2, 1)):
            assert not R.shape_ok(40, M2, K2, Ds2)
            raises(gpu, ERR_ARG, gpu.RefineLevel.from_arrays, idx, np.zeros((M2, K2, Ds2), dtype=np.float32), z[:, :M2])
        raises(gpu, ERR_ARG, gpu.RefineLevel.build, idx, v, M2=16, K2=16)
        raises(gpu, ERR_ARG, gpu.RefineLevel.build, idx, v[:, :30])                           # ceil(30 / 8) != 5
        raises(gpu, ERR_ARG, gpu.RefineLevel.build, idx, v[:100])                             # n_rows != n_local
        raises(gpu, ERR_ARG, gpu.RefineLevel.build, idx, v, vec_id=np.full(n, n, dtype=np.uint32), K2=16)
        raises(gpu, ERR_ARG, gpu.RefineLevel.from_arrays, idx, np.zeros((3, 7, 14), dtype=np.float32), z[:100, :3])
        bad = z[:, :3].copy()
        bad[77, 2] = 7                                                                        # a code byte >= K2
        raises(gpu, ERR_ARG, gpu.RefineLevel.from_arrays, idx, np.zeros((3, 7, 14), dtype=np.float32), bad)
        bad[77, 2] = 6
        gpu.RefineLevel.from_arrays(idx, np.zeros((3, 7, 14), dtype=np.float32), bad).close()
        with gpu.RefineLevel.from_arrays(idx, np.zeros((40, 2, 1), dtype=np.float32), z[:, :40]) as lvl:   # M2 = D1
            q = np.zeros((1, 40), dtype=np.float32)
            raises(gpu, ERR_ARG, lvl.rerank, q, np.zeros((1, 4), dtype=np.int32), 5)
            raises(gpu, ERR_ARG, lvl.rerank, q, np.zeros((1, 16385), dtype=np.int32), 1)
            assert lvl.query_batch_refined(q, n, 3)[0].shape == (1, 3)
            raises(gpu, ERR_TOPK, lvl.query_batch_refined, q, n + 1, 3)                      # n_cand above the codes


def composed_level(gpu, idx, rows, n_local, M2, K2, train_n, max_iters, seed, start="rows", restarts=0):
    """dpq_refine_build's definition, by the public calls."""
    inf = idx.info()
    D1 = inf["M"] * inf["Ds"]
    ids = reportable(inf["node_lo"], inf["node_hi"], inf["n_codes_total"], even_rule=True)
    pos = R.sample_positions(n_local, train_n)
    sample = gpu.RefineLevel.residuals(idx, ids[pos], rows[pos])
    cb2, _ = gpu.train_codebook(sample, M=M2, K=K2, max_iters=max_iters, seed=seed, start=start, restarts=max(restarts, 1))
    assert cb2.shape == (M2, K2, -(-D1 // M2))
    codes2 = gpu.encode_pq(gpu.RefineLevel.residuals(idx, ids, rows), cb2)
    return cb2, codes2


@pytest.mark.gpu
@pytest.mark.parametrize("with_map", [False, True])
def test_build_is_the_composition_of_public_calls(gpu, with_map):
    from deltapq_amd import synth
    n, M, Ds = 3001, 8, 4
    payload, codes1 = make_tree(n, M, 11, dup=False)
    cb1 = synth.make_codebook(M, 256, Ds, seed=12)
    v = make_vectors(cb1, codes1, 31, 13)
    rng = np.random.default_rng(14)
    if with_map:
        vec_id = rng.permutation(n + 50)[:n].astype(np.uint32)
        table = np.zeros((n + 50, 31), dtype=np.float32)
        table[vec_id] = v
    else:
        vec_id, table = None, v
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as idx:
        raises(gpu, ERR_STATE, gpu.RefineLevel.build, idx, table, vec_id=vec_id)
        idx.set_codebook(cb1)
        for M2, K2, train_n, iters, start, restarts in ((0, 0, 0, 0, "rows", 0), (4, 16, 700, 5, "kmeans++", 2), (3, 7, n, 3, "rows", 0)):
            with gpu.RefineLevel.build(idx, table, vec_id=vec_id, M2=M2, K2=K2, train_n=train_n, max_iters=iters, seed=5,
                                       start=start, restarts=restarts) as lvl:
                m2, k2 = M2 or M, K2 or 256
                tn = train_n or min(n, 256 * k2)
                cb2, codes2 = composed_level(gpu, idx, v, n, m2, k2, tn, iters or 25, 5, start, restarts)
                gcw, gc = lvl.arrays()
                assert (lvl.M2, lvl.K2) == (m2, k2)
                assert np.array_equal(bits(gcw), bits(cb2)) and np.array_equal(gc, codes2), (M2, K2, train_n)
                # ... which is what the restatement encodes, too
                assert np.array_equal(gc, R.encode2(R.residuals(v, cb1, codes1), cb2))
                with gpu.RefineLevel.from_arrays(idx, gcw, gc) as again:                   # create / get round trip
                    a, b = again.arrays()
                    assert np.array_equal(bits(a), bits(gcw)) and np.array_equal(b, gc)
        raises(gpu, ERR_ARG, gpu.RefineLevel.build, idx, table, vec_id=vec_id, train_n=n + 1)


@pytest.mark.gpu
def test_build_streams_a_second_slice(gpu):
    """n_local = 2^20 + 257: the nodes pass in two slices."""
    from deltapq_amd import synth
    n = (1 << 20) + 257
    tree = synth.synth_tree(n, 8, seed=21, mean_diffs=2.0)
    payload, _ = synth.encode_dtc(tree)
    cb1 = synth.make_codebook(8, 256, 1, seed=22)
    rng = np.random.default_rng(23)
    v = rng.normal(100.0, 40.0, size=(n, 8)).astype(np.float32)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256) as idx:
        idx.set_codebook(cb1)
        with gpu.RefineLevel.build(idx, v, M2=1, K2=2, max_iters=1, seed=3) as lvl:
            cb2, codes2 = composed_level(gpu, idx, v, n, 1, 2, 512, 1, 3)
            gcw, gc = lvl.arrays()
            assert np.array_equal(bits(gcw), bits(cb2))
            assert np.array_equal(gc, codes2)


@pytest.mark.gpu
def test_query_batch_refined_is_the_two_call_composition(gpu):
    from deltapq_amd import synth
    n, M, Ds, nq = 20001, 8, 16, 70
    payload, codes1 = make_tree(n, M, 31, dup=False)
    cb1 = synth.make_codebook(M, 256, Ds, seed=32)
    v = make_vectors(cb1, codes1, 127, 33)
    queries = synth.make_queries(nq, 128, seed=34)
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as idx:
        idx.set_codebook(cb1)
        before = idx.query_batch(queries, 10)
        with gpu.RefineLevel.build(idx, v, K2=16, train_n=2000, max_iters=4) as lvl:
            xrows = lvl.reconstruct(reportable(0, n, n))
            for n_cand, top_k in ((100, 10), (64, 64), (1, 1), (1000, 100)):
                ci, _ = idx.query_batch(queries, n_cand)
                want = lvl.rerank(queries, ci, top_k)
                assert same(lvl.query_batch_refined(queries, n_cand, top_k), want), (n_cand, top_k)
                assert same(want, R.rerank(xrows, queries, ci, top_k, n_total=n))
            # a filter that allows fewer than n_cand nodes: padded shortlists reach the re-rank
            allowed = np.random.default_rng(35).permutation(n)[:37].astype(np.int32)
            with gpu.IdFilter.from_ids(idx, allowed) as f:
                ci, _ = idx.query_batch_filtered(queries, 100, f)
                assert (ci[:, 37:] == -1).all() and (ci[:, :37] >= 0).all()
                want = lvl.rerank(queries, ci, 50)
                got = lvl.query_batch_refined(queries, 100, 50, id_filter=f)
                assert same(got, want) and (got[0][:, 37:] == -1).all() and np.isinf(got[1][:, 37:]).all()
                assert same(want, R.rerank(xrows, queries, ci, 50, n_total=n))
            raises(gpu, ERR_ARG, lvl.query_batch_refined, queries, 10, 11)
            assert same(idx.query_batch(queries, 10), before)                             # the plain call answers as before
            # a level of another handle
            with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as other:
                other.set_codebook(cb1)
                q = np.ascontiguousarray(queries, dtype=np.float32)
                oi, od = np.empty((nq, 5), dtype=np.int32), np.empty((nq, 5), dtype=np.float32)
                rc = lvl._lib.dpq_query_batch_refined(other._h, lvl._h, None, ctypes.c_void_p(q.ctypes.data), nq, 10, 5,
                                                      ctypes.c_void_p(oi.ctypes.data), ctypes.c_void_p(od.ctypes.data))
                assert rc == ERR_ARG
            # dpq_set_codebook again: the level keeps the codebook it was made with
            want = lvl.rerank(queries, ci, 50)
            idx.set_codebook(synth.make_codebook(M, 256, Ds, seed=99))
            assert same(lvl.rerank(queries, ci, 50), want)
            assert np.array_equal(bits(lvl.reconstruct(reportable(0, n, n))), bits(xrows))


def check_handle(gpu, idx, cb1, codes1, v, n_total, seed, even_rule=True):
    """A level over the nodes the handle holds (codes1, v: theirs), against the restatement; returns the x rows."""
    inf = idx.info()
    lo, hi = inf["node_lo"], inf["node_hi"]
    assert len(codes1) == len(v) == hi - lo
    cb2, codes2, res = make_level(cb1, codes1, v, 4, 16, seed)
    xrows = R.reconstruct(cb1, codes1, cb2, codes2)
    ids = reportable(lo, hi, n_total, even_rule)
    rng = np.random.default_rng(seed)
    queries = (xrows[rng.integers(0, hi - lo, size=5)] + rng.normal(0.0, 8.0, size=(5, xrows.shape[1]))).astype(np.float32)
    cand = make_candidates(ids, 5, 300, seed + 1)
    assert np.array_equal(bits(gpu.RefineLevel.residuals(idx, ids[:500], v[:500])), bits(res[:500]))
    with gpu.RefineLevel.from_arrays(idx, cb2, codes2) as lvl:
        assert np.array_equal(bits(lvl.reconstruct(ids[-300:])), bits(xrows[-300:]))
        want = R.rerank(xrows, queries, cand, 20, node_lo=lo, n_total=n_total, even_rule=even_rule)
        assert same(lvl.rerank(queries, cand, 20), want)
        for bad_id in (lo - 1, hi + 1, (n_total - 1) if (even_rule and n_total % 2 == 0 and hi == n_total) else hi):
            if bad_id < 0:
                continue
            bad = cand.copy()
            bad[2, 7] = bad_id
            raises(gpu, ERR_ARG, lvl.rerank, queries, bad, 20)
    return xrows


@pytest.mark.gpu
def test_shards_merge_over_the_union_of_shortlists(gpu):
    from deltapq_amd import synth
    n, M, Ds, nq, n_cand, top_k = 100002, 8, 4, 6, 50, 20
    payload, codes1 = make_tree(n, M, 41, dup=False)
    cb1 = synth.make_codebook(M, 256, Ds, seed=42)
    v = make_vectors(cb1, codes1, 31, 43)
    queries = (R.level1(cb1, codes1)[:nq] + 3.0).astype(np.float32)
    parts_i, parts_d, short, xall = [], [], [], np.zeros((n, 32), dtype=np.float32)
    for r in range(2):
        with gpu.DeltaPQIndex.open_memory(payload, n, M, 256, shard_rank=r, shard_count=2) as idx:
            idx.set_codebook(cb1)
            inf = idx.info()
            lo, hi = inf["node_lo"], inf["node_hi"]
            assert hi - lo > 40000
            xall[lo:hi] = check_handle(gpu, idx, cb1, codes1[lo:hi], v[lo:hi], n, seed=50 + r)
            cb2, codes2, _ = make_level(cb1, codes1[lo:hi], v[lo:hi], 4, 16, 50 + r)
            with gpu.RefineLevel.from_arrays(idx, cb2, codes2) as lvl:
                ci, _ = idx.query_batch(queries, n_cand)
                short.append(ci)
                i, d = lvl.query_batch_refined(queries, n_cand, top_k)
                parts_i.append(i)
                parts_d.append(d)
    merged = gpu.merge_topk_host(np.stack(parts_i), np.stack(parts_d))
    union = np.concatenate(short, axis=1)
    assert same(merged, R.rerank(xall, queries, union, top_k, n_total=n))


@pytest.mark.gpu
def test_parts_prefixes_and_plain_handles(gpu):
    from deltapq_amd import synth
    n, M, Ds = 7000, 8, 4
    payload, codes1 = make_tree(n, M, 61)
    cb1 = synth.make_codebook(M, 256, Ds, seed=62)
    v = make_vectors(cb1, codes1, 32, 63)
    off = 1000003
    for gn in (off + n, off + n + 11):                       # the part that ends an even index; a middle part
        with gpu.DeltaPQIndex.open_memory(payload, n, M, 256, global_offset=off, global_n_codes=gn) as idx:
            idx.set_codebook(cb1)
            assert idx.info()["node_lo"] == off
            check_handle(gpu, idx, cb1, codes1, v, gn, seed=gn % 97)
    for prefix in (5001, 5000):
        with gpu.DeltaPQIndex.open_memory(payload, n, M, 256, num_codes=prefix) as idx:
            idx.set_codebook(cb1)
            assert idx.info()["node_hi"] == prefix
            check_handle(gpu, idx, cb1, codes1[:prefix], v[:prefix], prefix, seed=prefix)
    rng = np.random.default_rng(64)
    for Mp in (8, 16):
        codes = rng.integers(0, 256, size=(4000, Mp), dtype=np.uint8)
        codes[1::2] = codes[::2]
        cbp = synth.make_codebook(Mp, 256, 2, seed=65)
        vp = make_vectors(cbp, codes, 2 * Mp, 66)
        with gpu.DeltaPQIndex.open_plain(codes) as idx:
            idx.set_codebook(cbp)
            check_handle(gpu, idx, cbp, codes, vp, 4000, seed=67, even_rule=False)


@pytest.mark.gpu
def test_cli_refine_and_recall(gpu, tmp_path):
    """learn -> encode -> approx_tree -> refine -> recall -refine on a small base: the printed recalls are those the
    Python API computes, and the written files load to the same level."""
    from deltapq_amd import synth
    d = str(tmp_path)
    n, nq, D, M, K, M2, K2, k, Rr = 3000, 40, 32, 8, 256, 4, 16, 10, 100
    base = synth.make_clustered_vectors(n, D, seed=71, n_clusters=60)
    queries = synth.make_clustered_vectors(nq, D, seed=72, n_clusters=60, centre_seed=71)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), queries)

    def run(*args):
        r = subprocess.run([EXE, "-dataset", d, "-ext", "fvecs", "-m", str(M), "-k", str(K), "-N", str(n)] + [str(a) for a in args],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    run("-task", "learn")
    run("-task", "encode")
    run("-task", "approx_tree", "-h", 1, "-diff", 8)
    run("-task", "groundtruth", "-topk", k, "-query_size", nq)
    out = run("-task", "refine", "-m2", M2, "-k2", K2, "-train_size", 2000, "-seed", 4)
    cw_path = os.path.join(d, "M%dK%d_refine_M%dK%dcodewords.txt" % (M, K, M2, K2))
    codes_path = os.path.join(d, "codes.bin.refine.M%dK%dM%dK%dN%d" % (M, K, M2, K2, n))
    assert os.path.exists(cw_path) and os.path.exists(codes_path), out
    cb1 = gpu.read_codewords(os.path.join(d, "M%dK%dcodewords.txt" % (M, K)))
    cb2 = gpu.read_codewords(cw_path)
    codes2 = gpu.read_codes_plain(codes_path, M2)
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M%dK%d_Approx_TreeNodesDFS_N%d" % (M, K, n)), n)
    n_codes, payload = gpu.read_dtc_file(synth.dtc_file_name(d, M, K, n))
    with gpu.DeltaPQIndex.open_memory(payload, n_codes, M, K) as idx:
        idx.set_codebook(cb1)
        with gpu.RefineLevel.build(idx, base, vec_id=vec_id, M2=M2, K2=K2, train_n=2000, seed=4) as lvl:
            gcw, gc = lvl.arrays()
            assert np.array_equal(bits(gcw), bits(cb2)) and np.array_equal(gc, codes2)   # the files hold this level
        with gpu.RefineLevel.from_arrays(idx, cb2, codes2) as lvl:
            pq_ids, _ = idx.query_batch(queries, k)
            ref_ids, _ = lvl.query_batch_refined(queries, Rr, k)
    with gpu.FlatIndex(base) as flat:
        truth, _ = flat.search(queries, k)
    to_vec = np.append(vec_id.astype(np.int64), vec_id[-1])          # (the even-N id of the last node)
    want_pq = gpu.recall(np.where(pq_ids >= 0, to_vec[pq_ids], -1).astype(np.int32), truth, k=k, R=k)
    want_ref = gpu.recall(np.where(ref_ids >= 0, to_vec[ref_ids], -1).astype(np.int32), truth, k=k, R=k)
    out = run("-task", "recall", "-topk", k, "-query_size", nq, "-refine", Rr, "-m2", M2, "-k2", K2)
    m = re.search(r"refine: recall@%d PQ ([0-9.]+) -> top-%d refined ([0-9.]+)" % (k, Rr), out)
    assert m, out
    assert abs(float(m.group(1)) - want_pq) < 5e-7 and abs(float(m.group(2)) - want_ref) < 5e-7, (out, want_pq, want_ref)
    assert want_ref >= want_pq
