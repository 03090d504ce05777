"""Exact search over raw vectors (dpq_flat_*, include/deltapq_amd.h): ground truth, recall, re-ranking.  The rules are
restated in _exact_restatement.py; the GPU is held to them bit for bit on ids and on distance bits -- the order
(distance, id) is total, so no tie slack is needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _exact_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
GOLDEN = os.path.join(ROOT, "tests", "golden", "groundtruth_reference_format.txt")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def order_vector():
    """D = 514, q = 0: in order the fp64 sum is 1 + 2^-24 exactly and every later 2^-60 is lost, so fp32 rounds to
    even (0x3f800000); reversed, pairwise or by partial sums the 512 small terms add up first and tip it to 0x3f800001."""
    v = np.empty(514, dtype=np.float32)
    v[0], v[1], v[2:] = 1.0, 2.0 ** -12, 2.0 ** -30
    return v


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_restatement_known_answer_pins_the_order():
    v = order_vector()
    q = np.zeros(514, dtype=np.float32)
    assert bits(X.distances(v[None, :], q))[0] == 0x3F800000
    assert bits(X.distances(v[None, ::-1], q))[0] == 0x3F800001      # the same terms, last dimension first
    acc = np.float64(0)
    for x in v:                                                       # a scalar loop agrees with the vectorised one
        t = np.float32(x - np.float32(0))
        acc += np.float64(np.float32(t * t))
    assert bits(np.float32(acc)) == 0x3F800000


def test_restatement_orders_by_distance_then_id():
    base = np.array([[2.0], [1.0], [-1.0], [3.0], [1.0]], dtype=np.float32)
    ids, d = X.search(base, np.zeros((1, 1), dtype=np.float32), 4, id_offset=10)
    assert ids.tolist() == [[11, 12, 14, 10]] and d.tolist() == [[1.0, 1.0, 1.0, 4.0]]
    ids, d = X.rerank(base, np.zeros((1, 1), dtype=np.float32), np.array([[13, -1, 14, 14, 11]]), 4, id_offset=10)
    assert ids.tolist() == [[11, 14, 13, -1]] and d.tolist() == [[1.0, 1.0, 9.0, np.inf]]


def _open_raw(lib, v, n, D, device=0, id_offset=0, out="alloc"):
    h = ctypes.c_void_p()
    ptr = None if v is None else ctypes.c_void_p(v.ctypes.data)
    rc = lib.dpq_flat_open(ptr, n, D, device, id_offset, None if out is None else ctypes.byref(h))
    return rc, h


def test_flat_open_argument_errors_come_before_any_device_call(lib):
    from deltapq_amd import api
    v = np.zeros((4, 8), dtype=np.float32)
    assert _open_raw(lib, None, 4, 8)[0] == -1
    assert _open_raw(lib, v, 4, 8, out=None)[0] == -1
    assert _open_raw(lib, v, 0, 8)[0] == -1
    assert _open_raw(lib, v, 4, 0)[0] == -1
    assert _open_raw(lib, v, 4, 2049)[0] == -1
    assert _open_raw(lib, v, 4, 8, id_offset=-1)[0] == -1
    assert _open_raw(lib, v, 4, 8, id_offset=2 ** 31 - 4)[0] == -1        # n + id_offset == 2^31
    assert b"dpq_flat_open" in lib.dpq_last_error()
    if api.device_count() == 0:                                            # ... and only then the device
        assert _open_raw(lib, v, 4, 8)[0] == -4
        with pytest.raises(api.DpqError) as e:
            api.FlatIndex(v)
        assert e.value.status == -4 and "no CPU fallback" in str(e.value)
    assert _open_raw(lib, v, 4, 8, device=10 ** 6)[0] == -4


@pytest.mark.parametrize("ext", ["fvecs", "bvecs"])
def test_read_vecs_range_equals_slices_of_read_vecs(lib, tmp_path, ext):
    from deltapq_amd import api, synth
    rng = np.random.default_rng(3)
    n, D = 37, 10
    if ext == "bvecs":
        v = rng.integers(0, 256, size=(n, D)).astype(np.float32)
        synth.write_bvecs(str(tmp_path / "v.bvecs"), v)
    else:
        v = rng.normal(size=(n, D)).astype(np.float32)
        synth.write_fvecs(str(tmp_path / "v.fvecs"), v)
    path = str(tmp_path / ("v." + ext))
    whole = api.read_vecs(path, ext)
    assert np.array_equal(bits(whole), bits(v))
    for first, count in ((0, n), (0, 1), (5, 20), (n - 1, 1), (n, 0), (12, 0)):
        got = api.read_vecs_range(path, first, count, ext)
        assert got.shape == (count, D) and np.array_equal(bits(got), bits(whole[first:first + count]))
    for first, count in ((0, n + 1), (n, 1), (30, 8)):
        with pytest.raises(api.DpqError) as e:
            api.read_vecs_range(path, first, count, ext)
        assert e.value.status == -2
    with pytest.raises(api.DpqError) as e:
        api.read_vecs_range(str(tmp_path / "absent"), 0, 1, ext)
    assert e.value.status == -2


def test_groundtruth_file_reads_back_the_same_bits(lib, tmp_path):
    from deltapq_amd import api
    rng = np.random.default_rng(5)
    d = np.array([[0.0, 0.1, 16777216.0, 16777218.0], [np.nextafter(np.float32(16777216), np.float32(0)), 1e-30, 3.4e38, 1.0]],
                 dtype=np.float32)
    d = np.concatenate([d, np.abs(rng.normal(size=(30, 4)) * 10.0 ** rng.uniform(-20, 20, size=(30, 4))).astype(np.float32)])
    ids = rng.integers(0, 2 ** 31 - 1, size=d.shape).astype(np.int32)
    path = str(tmp_path / "gt.txt")
    api.write_groundtruth(path, ids, d)
    text = open(path).read().splitlines()
    assert text[0] == "32,4" and len(text) == 33 and text[1].endswith(",") and text[1].count(",") == 8
    gi, gd = api.read_groundtruth(path)
    assert np.array_equal(gi, ids) and np.array_equal(bits(gd), bits(d))
    with pytest.raises(api.DpqError) as e:
        api.read_groundtruth(str(tmp_path / "absent.txt"))
    assert e.value.status == -2


def test_groundtruth_file_in_the_reference_format_is_read(lib):
    """tests/golden/groundtruth_reference_format.txt: written by hand as the reference writes it (six digits)."""
    from deltapq_amd import api
    ids, d = api.read_groundtruth(GOLDEN)
    assert ids.tolist() == [[7, 12, 3, 40], [0, 1, 2, 5], [9, 8, 11, 10]]
    want = np.array([[0, 0.25, 1.5e6, 3.40282e38], [1e-5, 0.1, 16777216, 1.67772e7], [2.5, 2.5, 100, 1e10]], dtype=np.float32)
    assert np.array_equal(bits(d), bits(want))


def test_recall_on_hand_counted_cases(lib):
    from deltapq_amd import api
    truth = np.array([[1, 2, 3, 4], [10, 11, 12, 13]], dtype=np.int32)
    found = np.array([[4, 9, 1, 7], [13, 12, 11, 10]], dtype=np.int32)
    assert api.recall(found, truth) == (2 + 4) / 8                      # R = k = 4
    assert api.recall(found, truth, k=2, R=2) == (0 + 0) / 4
    assert api.recall(found, truth, k=1, R=4) == (1 + 1) / 2            # 1-recall@4
    assert api.recall(found, truth, k=1, R=2) == 0.0
    f10 = np.array([[5, 6, 7, 8, 9, 20, 21, 22, 23, 1], [0] * 10], dtype=np.int32)
    assert api.recall(f10, truth, k=1, R=10) == 0.5                     # k = 1, R = 10
    assert api.recall(f10, truth, k=1, R=9) == 0.0
    padded = np.array([[1, -1, -1, -1], [-1, -1, -1, -1]], dtype=np.int32)
    assert api.recall(padded, truth) == 1 / 8                           # padding with -1 never counts
    tpad = np.array([[1, 2, -1, -1], [-1, -1, -1, -1]], dtype=np.int32)
    assert api.recall(padded, tpad) == 1 / 8
    assert api.recall(np.array([[1, 1, 1, 1], [10, 10, 11, 11]], dtype=np.int32), truth) == 3 / 8   # an id counts once
    wide = np.array([[1, 2, 3, 4, 99, 98], [10, 11, 12, 13, 97, 96]], dtype=np.int32)                # truth_stride > k
    assert api.recall(found, wide, k=4, R=4) == 6 / 8
    assert api.recall(np.array([[99, 98, 1, 2], [0, 0, 0, 0]], dtype=np.int32), wide, k=2, R=4) == 2 / 4
    for f, t, k, R in ((found, truth, 5, 4), (found, truth, 4, 5), (found, truth, 0, 4)):
        with pytest.raises(api.DpqError) as e:
            api.recall(f, t, k=k, R=R)
        assert e.value.status == -1
    for f, t in zip((found, f10, padded), (truth, truth, truth)):
        for k, R in ((4, 4), (1, f.shape[1]), (2, 3)):
            assert api.recall(f, t, k=k, R=R) == X.recall(f, t, k, R)


def test_cli_usage_of_the_new_tasks(built):
    r = subprocess.run([EXE, "-task", "groundtruth"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-task groundtruth" in r.stdout
    r = subprocess.run([EXE, "-task", "recall"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-task recall" in r.stdout and "-rerank" in r.stdout
    r = subprocess.run([EXE, "-task", "diff_scan"], capture_output=True, text=True)
    assert r.returncode == 2 and "groundtruth and recall are implemented" in r.stdout


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def assert_same(got, want, what):
    gi, gd = got
    wi, wd = want
    bad_i = int((gi != wi).sum())
    bad_d = int((bits(gd) != bits(wd)).sum())
    print("%s: %d of %d ids and %d of %d distance bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert bad_i == 0 and bad_d == 0, what


@pytest.mark.gpu
def test_gpu_known_answer_pins_the_order(gpu):
    v = order_vector()
    base = np.stack([v, v[::-1], np.zeros(514, dtype=np.float32)])
    with gpu.FlatIndex(base) as f:
        ids, d = f.search(np.zeros((1, 514), dtype=np.float32), 3)
        assert ids.tolist() == [[2, 0, 1]] and bits(d).tolist() == [[0, 0x3F800000, 0x3F800001]]
        ids, d = f.rerank(np.zeros((1, 514), dtype=np.float32), np.array([[1, 0]], dtype=np.int32), 2)
        assert ids.tolist() == [[0, 1]] and bits(d).tolist() == [[0x3F800000, 0x3F800001]]


@pytest.mark.gpu
def test_gpu_search_integer_data_with_ties(gpu):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 6, size=(5000, 128)).astype(np.float32)
    base[1000:2000] = base[0:1000]
    qs = base[[3, 500, 999, 4000]] + rng.integers(0, 2, size=(4, 128)).astype(np.float32)
    want = X.search(base, qs, 50)
    tied = sum(int((np.diff(bits(row)) == 0).sum()) for row in want[1])
    print("exactly tied neighbours in the restatement's lists:", tied)
    assert tied >= 3       # the copied rows tie pairwise
    with gpu.FlatIndex(base) as f:
        assert_same(f.search(qs, 50), want, "integer data with ties")


@pytest.mark.gpu
def test_gpu_search_wide_exponent_spread(gpu):
    rng = np.random.default_rng(12)
    base = (rng.normal(size=(20000, 128)) * 10.0 ** rng.uniform(-3, 3, size=(20000, 128))).astype(np.float32)
    qs = (rng.normal(size=(64, 128)) * 10.0 ** rng.uniform(-3, 3, size=(64, 128))).astype(np.float32)
    with gpu.FlatIndex(base) as f:
        assert_same(f.search(qs, 100), X.search(base, qs, 100), "wide exponent spread")


@pytest.mark.gpu
def test_gpu_search_every_stripe_lowers_the_threshold(gpu):
    """The base in descending distance to the first query: every vector beats the threshold so far."""
    rng = np.random.default_rng(13)
    base = rng.normal(size=(30000, 8)).astype(np.float32)
    qs = rng.normal(size=(2, 8)).astype(np.float32)
    base = base[np.argsort(-X.distances(base, qs[0]), kind="stable")]
    with gpu.FlatIndex(base) as f:
        assert_same(f.search(qs, 100), X.search(base, qs, 100), "descending order")
        assert_same(f.search(qs, 3000), X.search(base, qs, 3000), "descending order, top-3000")


@pytest.mark.gpu
@pytest.mark.parametrize("D,n,nq,top_k", [(1, 4099, 1, 1), (3, 4099, 65, 2048), (3, 4099, 1000, 1), (100, 10007, 3, 10000),
                                          (960, 4099, 5, 4099), (100, 4099, 65, 100)])
def test_gpu_search_shapes(gpu, D, n, nq, top_k):
    rng = np.random.default_rng(D * 7 + nq)
    base = rng.normal(size=(n, D)).astype(np.float32)
    qs = rng.normal(size=(nq, D)).astype(np.float32)
    with gpu.FlatIndex(base) as f:
        assert_same(f.search(qs, top_k), X.search(base, qs, top_k), "D %d n %d nq %d top-%d" % (D, n, nq, top_k))
        if top_k == n:
            with pytest.raises(gpu.DpqError) as e:
                f.search(qs, n + 1)
            assert e.value.status == -8
        ids, d = f.search(qs[:0], top_k)     # nq == 0 is fine
        assert ids.shape == (0, top_k)
        for bad in (0, 16385):
            with pytest.raises(gpu.DpqError) as e:
                f.search(qs, bad)
            assert e.value.status == -1


@pytest.mark.gpu
def test_gpu_search_offsets_and_parts(gpu):
    rng = np.random.default_rng(14)
    base = rng.integers(0, 4, size=(6001, 24)).astype(np.float32)    # many ties across the cut
    qs = rng.integers(0, 4, size=(9, 24)).astype(np.float32)
    k, cut = 300, 2500
    with gpu.FlatIndex(base, id_offset=1000) as f:
        whole = f.search(qs, k)
    assert_same(whole, X.search(base, qs, k, id_offset=1000), "id_offset")
    with gpu.FlatIndex(base[:cut], id_offset=1000) as a, gpu.FlatIndex(base[cut:], id_offset=1000 + cut) as b:
        ia, da = a.search(qs, k)
        ib, db = b.search(qs, k)
    assert_same(gpu.merge_topk_host(np.stack([ia, ib]), np.stack([da, db])), whole, "two parts merged")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand,top_k,D", [(1, 1, 128), (100, 100, 100), (100, 7, 128), (2048, 100, 128), (16384, 1000, 32)])
def test_gpu_rerank_matches_the_restatement(gpu, n_cand, top_k, D):
    import torch
    rng = np.random.default_rng(n_cand + top_k)
    n, nq, off = 5000, 7, 300
    base = rng.integers(0, 9, size=(n, D)).astype(np.float32) * np.float32(0.37)
    qs = rng.normal(size=(nq, D)).astype(np.float32)
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)     # with n_cand >= 100: duplicates
    cand[rng.random(size=cand.shape) < 0.2] = -1                               # padding
    if n_cand >= 100:
        cand[1, 5:] = -1                                                       # fewer valid candidates than top_k
        cand[2, :] = -1                                                        # none at all
        cand[3, :50] = cand[3, 50]
    with gpu.FlatIndex(base, id_offset=off) as f:
        want = X.rerank(base, qs, cand, top_k, id_offset=off)
        assert_same(f.rerank(qs, cand, top_k), want, "rerank n_cand %d" % n_cand)
        ti, td = f.rerank_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(cand).cuda(), top_k)
        assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "rerank on device tensors")
        if n_cand >= 100:
            assert (want[0][2] == -1).all() and np.isinf(want[1][2]).all() and (want[0][1] == -1).sum() >= top_k - 5
        for bad_id in (off - 1, off + n):                                      # names no row: both variants refuse
            bad = cand.copy()
            bad[nq - 1, n_cand - 1] = bad_id
            with pytest.raises(gpu.DpqError) as e:
                f.rerank(qs, bad, top_k)
            assert e.value.status == -1
            with pytest.raises(gpu.DpqError) as e:
                f.rerank_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(bad).cuda(), top_k)
            assert e.value.status == -1
        assert_same(f.rerank(qs, cand, top_k), want, "rerank after a refused call")
        if n_cand > 1:
            with pytest.raises(gpu.DpqError) as e:
                f.rerank(qs, cand, n_cand + 1)
            assert e.value.status == -1


@pytest.mark.gpu
def test_gpu_rerank_with_a_map_and_the_even_n_rule(gpu):
    rng = np.random.default_rng(15)
    n, n_map, D, nq, n_cand, k = 3000, 2000, 64, 5, 300, 40
    base = rng.normal(size=(n, D)).astype(np.float32)
    qs = rng.normal(size=(nq, D)).astype(np.float32)
    id_map = rng.permutation(n)[:n_map].astype(np.uint32)
    cand = rng.integers(0, n_map - 1, size=(nq, n_cand)).astype(np.int32)      # position n_map - 1 only through the rule
    cand[:, 7] = n_map                                                         # the even-N id of the last position
    cand[0, 8] = -1
    with gpu.FlatIndex(base, id_offset=50) as f:
        f.set_id_map(id_map)
        want = X.rerank(base, qs, cand, k, id_offset=50, id_map=id_map)
        assert_same(f.rerank(qs, cand, k), want, "rerank through a map")
        only = np.full((nq, 2), n_map, dtype=np.int32)
        ids, _ = f.rerank(qs, only, 1)
        assert (ids[:, 0] == int(id_map[n_map - 1]) + 50).all()
        bad = cand.copy()
        bad[2, 3] = n_map + 1
        with pytest.raises(gpu.DpqError) as e:
            f.rerank(qs, bad, k)
        assert e.value.status == -1
        with pytest.raises(gpu.DpqError) as e:
            f.set_id_map(np.array([0, n], dtype=np.uint32))
        assert e.value.status == -1
    with gpu.FlatIndex(base) as f:                                             # an odd map: n_map itself names nothing
        f.set_id_map(id_map[:n_map - 1])
        with pytest.raises(gpu.DpqError) as e:
            f.rerank(qs, np.full((nq, 2), n_map - 1, dtype=np.int32), 1)
        assert e.value.status == -1


def _positions_to_ids(pos, vec_id):
    n = len(vec_id)
    p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    return np.where(p >= 0, vec_id[np.clip(p, 0, n - 1)].astype(np.int64), -1).astype(np.int32)


def _build_index(gpu, base):
    cb, _ = gpu.train_codebook(base, M=8, K=256, max_iters=6, seed=1)
    codes = gpu.encode_pq(base, cb)
    tree = gpu.DeltaTree(codes, codebook=cb, device=0)
    return cb, tree


@pytest.mark.gpu
def test_gpu_end_to_end_rerank_does_not_lose_recall(gpu):
    from deltapq_amd import synth
    n, nq, k, R = 20000, 50, 10, 100
    base = synth.make_clustered_vectors(n, 128, seed=51, n_clusters=150, centre_seed=50)
    qs = synth.make_clustered_vectors(nq, 128, seed=52, n_clusters=150, centre_seed=50)
    cb, tree = _build_index(gpu, base)
    with gpu.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0) as idx, gpu.FlatIndex(base) as f:
        idx.set_codebook(cb)
        pos, _ = idx.query_batch(qs, R)
        truth, truth_d = f.search(qs, k)
        f.set_id_map(tree.vec_id)
        ri, rd = f.rerank(qs, pos, k)
    found = _positions_to_ids(pos, tree.vec_id)
    pq_recall = gpu.recall(found, truth, k=k, R=k)
    re_recall = gpu.recall(ri, truth, k=k, R=k)
    print("recall@%d of the PQ answer %.4f, re-ranked from top-%d %.4f" % (k, pq_recall, R, re_recall))
    assert re_recall >= pq_recall
    assert_same((ri, rd), X.rerank(base, qs, pos, k, id_map=tree.vec_id), "re-rank of the PQ answer")
    assert pq_recall == X.recall(found, truth, k, k)


@pytest.mark.gpu
def test_gpu_end_to_end_rerank_of_everything_is_the_exact_answer(gpu):
    from deltapq_amd import synth
    n, nq, k = 2000, 20, 10
    base = synth.make_clustered_vectors(n, 128, seed=61, n_clusters=40, centre_seed=60)
    qs = synth.make_clustered_vectors(nq, 128, seed=62, n_clusters=40, centre_seed=60)
    cb, tree = _build_index(gpu, base)
    with gpu.DeltaPQIndex.open_memory(tree.payload(), n, 8, 256, device=0) as idx, gpu.FlatIndex(base) as f:
        idx.set_codebook(cb)
        pos, _ = idx.query_batch(qs, n)
        truth = f.search(qs, k)
        f.set_id_map(tree.vec_id)
        got = f.rerank(qs, pos, k)
    assert_same(got, truth, "re-rank of all n candidates")
    assert gpu.recall(got[0], truth[0]) == 1.0


@pytest.mark.gpu
def test_gpu_cli_chain_groundtruth_and_recall(gpu, tmp_path):
    from deltapq_amd import synth
    d, n, nq, k, R = str(tmp_path), 5000, 16, 20, 200
    learn = synth.make_clustered_vectors(6000, 128, seed=71, n_clusters=150, centre_seed=70)
    base = synth.make_clustered_vectors(n, 128, seed=72, n_clusters=150, centre_seed=70)
    qs = synth.make_clustered_vectors(nq, 128, seed=73, n_clusters=150, centre_seed=70)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), learn)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), qs)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    env = dict(os.environ, DPQ_DEV="1", DPQ_GT_PART_ROWS="1800")      # three parts of the base
    outs = {}
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)],
                 ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-rerank", str(R)]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300, env=env if args[1] == "groundtruth" else None)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr   # a failed step ends the chain
        outs[args[1]] = r.stdout
    assert "in 3 part(s)" in outs["groundtruth"]
    gt_path = os.path.join(d, "groundtruth", "N%dTop%d.txt" % (n, k))
    assert gt_path in outs["groundtruth"]
    truth = gpu.read_groundtruth(gt_path)
    with gpu.FlatIndex(base) as f:
        assert_same(truth, f.search(qs, k), "ground-truth file")
        cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
        n_codes, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
        vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n), n)
        with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
            idx.set_codebook(cb)
            pos, _ = idx.query_batch(qs, R)
        f.set_id_map(vec_id)
        ri, _ = f.rerank(qs, pos, k)
    want_pq = gpu.recall(_positions_to_ids(pos, vec_id), truth[0], k=k, R=k)
    want_re = gpu.recall(ri, truth[0], k=k, R=k)
    got_pq = re.search(r"^recall@%d = ([0-9.]+)$" % k, outs["recall"], re.M)
    got_re = re.search(r"^reranked recall@%d = ([0-9.]+)$" % k, outs["recall"], re.M)
    assert got_pq and got_re, outs["recall"]
    print("CLI:", got_pq.group(0), "|", got_re.group(0), "| API: %.6f %.6f" % (want_pq, want_re))
    assert got_pq.group(1) == "%.6f" % want_pq and got_re.group(1) == "%.6f" % want_re
    assert want_re >= want_pq
    r = subprocess.run(common + ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-gt_topk", "5"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "-gt_topk" in r.stdout
