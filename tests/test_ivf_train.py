"""IVF training (dpq_ivf_train, dpq_ivf_assign[_device], dpq_write_vecs): the coarse quantiser's centroids, learned and
applied on the GPU.

GPU: strictly against tests/_ivf_train_restatement.py -- centroid bytes, labels, distance bits, iters_run, converged,
reseeded -- at the tile edges of the arg-min kernel (64 rows x 64 centroids x 32 dimensions), with exact ties, duplicated
centroids and vectors, distances that overflow, empty lists, nlist above the PQ trainer's 256 and nlist == n; against
dpq_ivf_build's labels on a DTC handle; end to end through IVF.train and the command line.  The one tolerance is the
distortion's: two fp64 sums of n non-negative terms in different orders differ by at most n * 2^-52 relative; on the hand
case the sums are exact and must be equal.  CPU: the symbols, the hand cases on the restatement, the argument checks.
Nothing is skipped and no case is exempt.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _ivf_restatement as I
import _ivf_train_restatement as R
import _numeric_edges as ne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
ERR_ARG = -1
SYMBOLS = ("dpq_ivf_train", "dpq_ivf_assign", "dpq_ivf_assign_device", "dpq_write_vecs")

HAND_POINTS = np.array([[0.0], [10.0], [2.5], [7.5], [5.0], [5.0]], dtype=np.float32)
HAND_INIT = np.array([[5.0], [1000.0]], dtype=np.float32)
HAND_CENTROIDS = np.array([[6.875], [1.25]], dtype=np.float32)
HAND_DISTORTION = [62.5, 37.5, 26.5, 20.3125]
# fp64 accumulation tells 16777218 from 16777216; dpq_train_codebook's fp32 accumulation gives 16777216 twice
SEP_VECTOR = np.zeros((1, 3), dtype=np.float32)
SEP_CENTROIDS = np.array([[4096.0, 1.0, 1.0], [4096.0, 1.0, 0.0]], dtype=np.float32)

SHAPES = [(1, 1, 1), (63, 2, 3), (64, 64, 32), (65, 65, 33), (129, 63, 31), (301, 130, 100), (700, 130, 33), (1500, 300, 8),
          (4097, 65, 128)]
# wider than a few slices of 32 dimensions: a width padded from 129 to 132, and one that ends in half a slice
WIDE_SHAPES = [(130, 70, 129), (200, 65, 176)]


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_hand_case(train):
    """tests/test_train_codebook.py's hand case (D = 1, where both distance rules agree): round 1 leaves list 1 empty and
    the lower of two equally far vectors donates; round 2 has an exact tie that the lower list wins; round 4 changes
    nothing and stops without an update."""
    c, st = train(HAND_POINTS, 2, 25, HAND_INIT)
    assert np.array_equal(c, HAND_CENTROIDS), c
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (4, 1, 1), st
    assert list(st["distortion"]) == HAND_DISTORTION, st["distortion"]
    c, st = train(HAND_POINTS, 2, 3, HAND_INIT)
    assert np.array_equal(c, HAND_CENTROIDS), c
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (3, 0, 1), st
    assert list(st["distortion"]) == HAND_DISTORTION[:3], st["distortion"]
    c, st = train(HAND_POINTS, 2, 1, HAND_INIT)
    assert np.array_equal(c, np.array([[5.0], [0.0]], dtype=np.float32)), c
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (1, 0, 1), st


def check_trained(gpu, v, nlist, what, **opts):
    """dpq_ivf_train against the restatement; returns both answers."""
    want_c, want = R.train(v, nlist, **opts)
    got_c, got = gpu.train_ivf_centroids(v, nlist, **opts)
    print("%s: iters_run %d / %d, converged %d / %d, reseeded %d / %d" % (
        what, got["iters_run"], want["iters_run"], got["converged"], want["converged"], got["reseeded"], want["reseeded"]))
    assert (got["iters_run"], got["converged"], got["reseeded"]) == (want["iters_run"], want["converged"], want["reseeded"]), what
    assert np.array_equal(bits(got_c), bits(want_c)), what + ": centroid bytes"
    assert len(got["distortion"]) == len(want["distortion"])
    for r, (a, b) in enumerate(zip(got["distortion"], want["distortion"])):
        assert a == b or abs(a - b) <= R.distortion_bound(len(v), b), "%s: distortion of round %d: %r, %r" % (what, r + 1, a, b)
    return got_c, got, want_c, want


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_the_symbols_are_declared_exported_and_bound(lib):
    from deltapq_amd import _lib
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared"
        assert name in exported, name + " is not exported"
        assert name in bound and hasattr(lib, name), name + " is not bound"
    assert ctypes.sizeof(_lib.IvfTrainOpts) == 2 * 4 + 8 + 4 * 4
    assert ctypes.sizeof(_lib.IvfTrainStats) == 2 * 4 + 8 + 64 * 8 + 6 * 8
    assert "IndexIVF::train" in header and "quantizer->assign" in header


def test_restatement_on_the_hand_case():
    check_hand_case(lambda v, nlist, it, init: R.train(v, nlist, max_iters=it, init=init))
    lab, win = R.assign(HAND_POINTS, np.array([[5.0], [0.0]], dtype=np.float32))
    assert lab.tolist() == [1, 0, 0, 0, 0, 0] and win.tolist() == [0.0, 25.0, 6.25, 6.25, 0.0, 0.0]


def test_restatement_on_the_rule_separating_case():
    """(0, 0, 0) against (4096, 1, 1) and (4096, 1, 0): 16777218 and 16777216 under the exact search's fp64 accumulation,
    so the label is 1; under dpq_train_codebook's fp32 accumulation both are 16777216 and list 0 would win the tie."""
    import _kmeans_restatement as K
    lab, win = R.assign(SEP_VECTOR, SEP_CENTROIDS)
    assert lab.tolist() == [1] and win.tolist() == [16777216.0]
    from _exact_restatement import distances
    assert distances(SEP_CENTROIDS, SEP_VECTOR[0]).tolist() == [16777218.0, 16777216.0]
    lab32, win32 = K.assign(SEP_VECTOR, SEP_CENTROIDS)
    assert lab32.tolist() == [0] and win32.tolist() == [16777216.0]


def test_argument_errors_need_no_device(lib, tmp_path):
    from deltapq_amd import _lib
    v = np.zeros((8, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.float32)
    lab = np.zeros(8, dtype=np.int32)
    d = np.zeros(8, dtype=np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    BIG = 1 << 31

    def opts(**kw):
        o = _lib.IvfTrainOpts(device=0, max_iters=5, seed=0, use_initial=0)
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def reserved(i):
        o = opts()
        o.reserved[i] = 1
        return o

    train = lambda vv=P(v), n=8, D=4, nlist=2, o=None, cc=P(c): lib.dpq_ivf_train(vv, n, D, nlist, o, cc, None)
    for what, rc in (("NULL vectors", train(vv=None)), ("NULL centroids", train(cc=None)), ("D = 0", train(D=0)),
                     ("D = 2049", train(D=2049)), ("nlist = 0", train(nlist=0)), ("nlist = 65537", train(nlist=65537, n=70000)),
                     ("nlist > n", train(nlist=9)), ("n = 0", train(n=0)), ("n = 2^31", train(n=BIG)),
                     ("max_iters = 0", train(o=opts(max_iters=0))), ("max_iters = 65", train(o=opts(max_iters=65))),
                     ("reserved[0]", train(o=reserved(0))), ("reserved[2]", train(o=reserved(2)))):
        assert rc == ERR_ARG, what
        assert b"dpq_ivf_train" in lib.dpq_last_error(), what
    assign = lambda cc=P(c), nlist=2, D=4, vv=P(v), n=8, ll=P(lab): lib.dpq_ivf_assign(cc, nlist, D, vv, n, 0, ll, P(d))
    for what, rc in (("NULL centroids", assign(cc=None)), ("NULL vectors", assign(vv=None)), ("NULL labels", assign(ll=None)),
                     ("D = 0", assign(D=0)), ("D = 2049", assign(D=2049)), ("nlist = 0", assign(nlist=0)),
                     ("nlist = 65537", assign(nlist=65537)), ("n = -1", assign(n=-1)), ("n = 2^31", assign(n=BIG))):
        assert rc == ERR_ARG, what
    # the device form never dereferences: aligned fakes, then what only it refuses
    fc, fv, fl = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    dev = lambda cc=fc, nlist=2, D=4, vv=fv, n=8, ll=fl: lib.dpq_ivf_assign_device(cc, nlist, D, vv, n, ll, None, None)
    for what, rc in (("NULL centroids", dev(cc=None)), ("NULL vectors", dev(vv=None)), ("NULL labels", dev(ll=None)),
                     ("D = 0", dev(D=0)), ("D = 2052", dev(D=2052)), ("nlist = 0", dev(nlist=0)),
                     ("nlist = 65537", dev(nlist=65537)), ("n = -1", dev(n=-1)), ("n = 2^31", dev(n=BIG)),
                     ("D % 4", dev(D=6)), ("misaligned centroids", dev(cc=ctypes.c_void_p(0x10004))),
                     ("misaligned vectors", dev(vv=ctypes.c_void_p(0x20008)))):
        assert rc == ERR_ARG, what
    assert lib.dpq_write_vecs(None, P(v), 8, 4) == ERR_ARG
    assert lib.dpq_write_vecs(str(tmp_path / "x.fvecs").encode(), None, 8, 4) == ERR_ARG
    assert lib.dpq_write_vecs(str(tmp_path / "x.fvecs").encode(), P(v), -1, 4) == ERR_ARG
    assert lib.dpq_write_vecs(str(tmp_path / "x.fvecs").encode(), P(v), 8, 0) == ERR_ARG


def test_write_vecs_is_what_read_vecs_reads(lib, tmp_path):
    from deltapq_amd import api, synth
    v = np.random.default_rng(3).normal(size=(7, 5)).astype(np.float32)
    v[0, 0], v[1, 1] = -0.0, np.float32(1e-45)
    path = str(tmp_path / "c.fvecs")
    api.write_vecs(path, v)
    assert np.array_equal(bits(api.read_vecs(path)), bits(v))
    synth.write_fvecs(str(tmp_path / "s.fvecs"), v)
    assert open(path, "rb").read() == open(str(tmp_path / "s.fvecs"), "rb").read()


# ---- GPU: the hand cases ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_hand_cases(gpu):
    check_hand_case(lambda v, nlist, it, init: gpu.train_ivf_centroids(v, nlist, max_iters=it, init=init))
    lab, win = gpu.ivf_assign(np.array([[5.0], [0.0]], dtype=np.float32), HAND_POINTS)
    assert lab.tolist() == [1, 0, 0, 0, 0, 0] and win.tolist() == [0.0, 25.0, 6.25, 6.25, 0.0, 0.0]
    lab, win = gpu.ivf_assign(SEP_CENTROIDS, SEP_VECTOR)
    assert lab.tolist() == [1] and win.tolist() == [16777216.0]
    lab, win = gpu.ivf_assign(SEP_CENTROIDS[::-1], SEP_VECTOR)
    assert lab.tolist() == [0] and win.tolist() == [16777216.0]
    assert gpu.ivf_assign(SEP_CENTROIDS, np.zeros((0, 3), dtype=np.float32))[0].shape == (0,)


# ---- GPU: assignment at the tile edges -------------------------------------------------------------------------------------

def assign_case(n, nlist, D, kind):
    rng = np.random.default_rng(1000 * n + 10 * nlist + D + (kind == "ints"))
    if kind == "ints":      # exact distance ties are common
        v = rng.integers(-3, 4, size=(n, D)).astype(np.float32)
        c = rng.integers(-3, 4, size=(nlist, D)).astype(np.float32)
    else:
        v = rng.normal(size=(n, D)).astype(np.float32)
        c = rng.normal(size=(nlist, D)).astype(np.float32)
    if nlist > 5:
        c[5] = c[2]          # a copy: the lower list wins every tie between them
    if n > 2:
        v[n // 2] = v[0]     # duplicated vectors, one of them in the last tile
        v[n - 1] = v[1]
    if nlist > 2 and n > 3:
        v[3] = c[nlist - 1]  # distance +0.0 to the last list
    return v, c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gauss", "ints"])
@pytest.mark.parametrize("shape", SHAPES + WIDE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gpu_assign_at_the_tile_edges(gpu, shape, kind):
    n, nlist, D = shape
    v, c = assign_case(n, nlist, D, kind)
    want_lab, want_win = R.assign(v, c)
    lab, win = gpu.ivf_assign(c, v)
    assert lab.dtype == np.int32 and np.array_equal(lab, want_lab), np.flatnonzero(lab != want_lab)[:8]
    assert np.array_equal(bits(win), bits(want_win))
    if nlist > 5:
        assert not np.any(lab == 5) and not np.any(want_lab == 5)
    if n > 2:
        assert lab[n // 2] == lab[0] and lab[n - 1] == lab[1]
    if kind == "ints" and nlist >= 63 and D <= 8:
        d = np.stack([I.E.distances(v, cc) for cc in c], axis=1)
        assert np.any((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1), "no exact tie in the data"


@pytest.mark.gpu
def test_gpu_assign_when_distances_overflow(gpu):
    """Entries of 2e19: every square is +inf in fp32, so every key is +inf << 32 | list and list 0 wins."""
    n, nlist, D = 65, 65, 33
    v, c = assign_case(n, nlist, D, "gauss")
    v[7] = 2e19
    v[64, 32] = -2e19
    want_lab, want_win = R.assign(v, c)
    assert want_lab[7] == 0 and want_lab[64] == 0 and np.isposinf(want_win[7]) and np.isposinf(want_win[64])
    lab, win = gpu.ivf_assign(c, v)
    assert np.array_equal(lab, want_lab) and np.array_equal(bits(win), bits(want_win))


# ---- GPU: training ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,nlist,D,iters", [(301, 7, 5, 25), (700, 130, 33, 25), (1500, 300, 8, 25), (4097, 65, 128, 4),
                                             (64, 64, 4, 25), (300, 20, 130, 6)])
def test_gpu_train_is_the_restatement(gpu, n, nlist, D, iters):
    v = np.random.default_rng(n + nlist).normal(size=(n, D)).astype(np.float32)
    check_trained(gpu, v, nlist, "%d x %d x %d" % (n, nlist, D), max_iters=iters, seed=n)


@pytest.mark.gpu
def test_gpu_train_converges_on_clustered_vectors(gpu):
    from deltapq_amd import synth
    v = synth.make_clustered_vectors(600, 16, seed=5, n_clusters=8)
    _, got, _, want = check_trained(gpu, v, 8, "clustered", max_iters=25, seed=2)
    d = got["distortion"]
    assert all(b <= a for a, b in zip(d, d[1:])), d      # Lloyd's rounds never raise the distortion
    assert want["converged"] == 1 or want["iters_run"] == 25


@pytest.mark.gpu
def test_gpu_train_repairs_empty_lists(gpu):
    """Four identical start centroids and one far away: lists 1..3 lose every tie to list 0, so E >= 3 in round one; the
    data's duplicated rows share their winning distance, and the index-ascending rule picks the donors."""
    rng = np.random.default_rng(8)
    v = rng.normal(size=(200, 6)).astype(np.float32)
    v[100:] = v[:100]                                    # every row twice: equal winning distances in pairs
    init = np.zeros((5, 6), dtype=np.float32)
    init[4] = 1000.0
    want_c, want = R.train(v, 5, max_iters=1, init=init)
    lab, win = R.assign(v, init)
    assert np.all(lab == 0) and want["reseeded"] == 4
    rank = np.lexsort((np.arange(200), -win.astype(np.float64)))
    assert rank[0] + 100 == rank[1] and rank[2] + 100 == rank[3]    # the duplicate follows its original
    assert np.array_equal(want_c[1:], v[rank[:4]])
    got_c, got = gpu.train_ivf_centroids(v, 5, max_iters=1, init=init)
    assert got["reseeded"] == 4 and np.array_equal(bits(got_c), bits(want_c))
    _, got, _, want = check_trained(gpu, v, 5, "empty lists", max_iters=25, init=init)
    assert got["reseeded"] >= 4


@pytest.mark.gpu
def test_gpu_train_is_deterministic_and_seeded(gpu):
    v = np.random.default_rng(12).normal(size=(900, 12)).astype(np.float32)
    a_c, a = gpu.train_ivf_centroids(v, 40, max_iters=6, seed=3)
    b_c, b = gpu.train_ivf_centroids(v, 40, max_iters=6, seed=3)
    assert np.array_equal(bits(a_c), bits(b_c))
    assert np.array_equal(np.array(a["distortion"]).view(np.uint64), np.array(b["distortion"]).view(np.uint64))
    c_c, _ = gpu.train_ivf_centroids(v, 40, max_iters=6, seed=4)
    assert not np.array_equal(a_c, c_c) and R.seeded_rows(900, 40, 3) != R.seeded_rows(900, 40, 4)
    # one round is one update of the seeded rows
    start = v[R.seeded_rows(900, 40, 3)]
    lab, win = R.assign(v, start)
    want, _ = R.update(v, lab, win, start)
    one, st = gpu.train_ivf_centroids(v, 40, max_iters=1, seed=3)
    assert np.array_equal(bits(one), bits(want)) and (st["iters_run"], st["converged"]) == (1, 0)
    # and the default options are 25 rounds from seed 0
    d_c = np.zeros((40, 12), dtype=np.float32)
    assert gpu._lib.load().dpq_ivf_train(ctypes.c_void_p(v.ctypes.data), 900, 12, 40, None, ctypes.c_void_p(d_c.ctypes.data),
                                         None) == 0
    assert np.array_equal(bits(d_c), bits(gpu.train_ivf_centroids(v, 40)[0]))


# ---- GPU: the device form --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_assign_device_form(gpu):
    import torch
    n, nlist, D = 700, 130, 32
    v, c = assign_case(n, nlist, D, "ints")
    host = gpu.ivf_assign(c, v)
    assert np.array_equal(host[0], R.assign(v, c)[0])
    tv, tc = torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda()
    lab, win = gpu.ivf_assign_torch(tc, tv)
    assert np.array_equal(lab.cpu().numpy(), host[0]) and np.array_equal(bits(win.cpu().numpy()), bits(host[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out_l = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out_d = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(side):
        got = gpu.ivf_assign_torch(tc, tv, out_labels=out_l, out_dists=out_d)
    side.synchronize()
    assert got[0] is out_l and got[1] is out_d
    assert np.array_equal(out_l.cpu().numpy(), host[0]) and np.array_equal(bits(out_d.cpu().numpy()), bits(host[1]))
    # what only the device form refuses
    lib = gpu._lib.load()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    assert lib.dpq_ivf_assign_device(P(tc), nlist, 30, P(tv), n, P(out_l), P(out_d), None) == ERR_ARG
    assert lib.dpq_ivf_assign_device(P(tc, 4), nlist - 1, D, P(tv), n, P(out_l), P(out_d), None) == ERR_ARG
    assert lib.dpq_ivf_assign_device(P(tc), nlist, D, P(tv, 8), n - 1, P(out_l), P(out_d), None) == ERR_ARG
    assert lib.dpq_ivf_assign_device(P(tc), nlist, D, P(tv), 0, P(out_l), P(out_d), None) == 0
    assert lib.dpq_ivf_assign_device(P(tc), nlist, D, P(tv), n, P(out_l), None, None) == 0     # no distances wanted
    torch.cuda.synchronize()
    assert np.array_equal(out_l.cpu().numpy(), host[0])


# ---- GPU: against the existing path, and end to end ------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_assign_gives_the_lists_of_ivf_build(gpu):
    from deltapq_amd import synth
    n, M, Ds, nlist = ne.N_SCAN, 8, 4, 9
    cb = synth.make_codebook(M, 256, Ds, seed=21)
    payload, _ = synth.encode_dtc(synth.synth_tree(n, M, seed=22))
    with gpu.DeltaPQIndex.open_memory(payload, n, M, 256) as idx:
        idx.set_codebook(cb)
        recon = idx.reconstruct(I.reported_ids(0, n))
        rng = np.random.default_rng(23)
        cents = recon[rng.choice(n, size=nlist, replace=False)].copy()
        cents[1::2] += rng.normal(size=(nlist // 2, M * Ds)).astype(np.float32)
        cents[7] = cents[2]
        labels, _ = gpu.ivf_assign(cents, recon)
        assert not np.any(labels == 7)
        with gpu.IVF.build(idx, cents) as built, gpu.IVF.from_labels(idx, labels, nlist) as mine:
            want, got = built.lists(), mine.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.gpu
def test_gpu_ivf_train_end_to_end(gpu):
    from deltapq_amd import synth
    n, D, M, nlist, k = 2000, 32, 8, 8, 10
    v = synth.make_clustered_vectors(n, D, seed=31, n_clusters=40, centre_seed=30)
    qs = synth.make_clustered_vectors(12, D, seed=32, n_clusters=40, centre_seed=30)
    cb, _ = gpu.train_codebook(v, M=M, K=256, max_iters=4)
    tree = gpu.DeltaTree(gpu.encode_pq(v, cb), 256, 1, cb)
    with gpu.DeltaPQIndex.open_memory(tree.payload(), n, M, 256) as idx:
        idx.set_codebook(cb)
        with gpu.IVF.train(idx, v, tree.vec_id, nlist, max_iters=10, seed=1) as ivf:
            inf = ivf.info()
            assert (inf["n_assigned"], inf["n_unassigned"], inf["nlist"], inf["has_centroids"]) == (n, 0, nlist, 1)
            want_c, _ = R.train(v, nlist, max_iters=10, seed=1)
            labels = R.assign(v, want_c)[0][tree.vec_id.astype(np.int64)]
            want = I.lists_from_labels(labels, nlist, even_rule=True)
            got = ivf.lists()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            a, b = ivf.search(qs, nlist, k), idx.query_batch(qs, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    tree.close()


@pytest.mark.gpu
def test_gpu_cli_ivf_learn_feeds_recall(gpu, tmp_path):
    """tests/test_ivf_search.py's chain with -task ivf_learn in place of the hand-made centroid file."""
    from deltapq_amd import synth
    d, n, nq, k, nlist = str(tmp_path), 2000, 12, 10, 8
    base = synth.make_clustered_vectors(n, 128, seed=91, n_clusters=60, centre_seed=90)
    qs = synth.make_clustered_vectors(nq, 128, seed=92, n_clusters=60, centre_seed=90)
    for name, vecs in (("learn", base), ("base", base), ("query", qs)):
        synth.write_fvecs(os.path.join(d, name + ".fvecs"), vecs)
    cents = os.path.join(d, "IVF%dcentroids.fvecs" % nlist)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    recall = ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-ivf", cents]
    outs = []
    for args in (["-task", "learn"], ["-task", "ivf_learn", "-nlist", str(nlist), "-iters", "6", "-seed", "4"],
                 ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)], recall + ["-nprobe", str(nlist)]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr    # a failed step ends the chain
        outs.append(r.stdout)
    want_c, want = R.train(base, nlist, max_iters=6, seed=4)
    assert np.array_equal(bits(gpu.read_vecs(cents)), bits(want_c))
    assert len(re.findall(r"^round \d+ distortion ", outs[1], re.M)) == want["iters_run"]
    assert re.search(r"^assign [0-9.e+-]+ \[ms\] update ", outs[1], re.M) and "-> " + cents in outs[1]
    plain = re.search(r"^recall@%d = ([0-9.]+)$" % k, r.stdout, re.M)
    ivf = re.search(r"^ivf recall@%d = ([0-9.]+) \(nlist %d, nprobe %d\)$" % (k, nlist, nlist), r.stdout, re.M)
    assert plain and ivf, r.stdout
    assert ivf.group(1) == plain.group(1) and float(plain.group(1)) > 0.2
    r = subprocess.run([EXE, "-dataset", d, "-task", "ivf_learn"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: deltapq -dataset DIR -task ivf_learn -nlist L" in r.stdout
