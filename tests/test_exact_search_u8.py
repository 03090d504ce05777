"""Exact search over byte vectors (dpq_flat_*_u8, include/deltapq_amd.h): the int8 matrix-core path is held bit for bit,
ids and distance bits, to the integer restatement in _exact_u8_restatement.py and to the fp32 path on the widened data."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _exact_restatement as X
import _exact_u8_restatement as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rounding_pair():
    """D = 260, zero query, 8 rows.  Row 5: 259 dimensions of 255, integer distance 16 841 475, exactly halfway between
    the floats 16 841 474 and 16 841 476 -- round to even gives the upper one.  Row 3: the same plus one dimension of 1,
    16 841 476 exactly.  Both report np.float32(16841476) and the list starts [3, 5]: id order, against integer order."""
    base = np.full((8, 260), 255, dtype=np.uint8)     # the other rows: 260 * 65025 = 16 906 500, farther
    base[5, 259] = 0
    base[3, 259] = 1
    return base, np.zeros((1, 260), dtype=np.uint8)


def assert_same(got, want, what):
    gi, gd = got
    wi, wd = want
    bad_i = int((gi != wi).sum())
    bad_d = int((bits(gd) != bits(wd)).sum())
    print("%s: %d of %d ids and %d of %d distance bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert bad_i == 0 and bad_d == 0, what


# ---- CPU ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [3, 260])
def test_restatements_agree(D):
    rng = np.random.default_rng(D)
    base = rng.integers(0, 256, size=(500, D)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(4, D)).astype(np.uint8)
    if D == 260:
        pair, zero = rounding_pair()
        base[:8], qs[0] = pair, zero[0]
        ids, d = U.search(pair, zero, 2)
        assert ids.tolist() == [[3, 5]] and bits(d).tolist() == [[int(np.float32(16841476).view(np.uint32))] * 2]
    for k in (1, 100, 500):
        assert_same(U.search(base, qs, k, id_offset=7), X.search(base.astype(np.float32), qs.astype(np.float32), k, id_offset=7),
                    "integer restatement against the fp32 one, top-%d" % k)


def _open_raw(lib, v, n, D, device=0, id_offset=0, out="alloc"):
    h = ctypes.c_void_p()
    ptr = None if v is None else ctypes.c_void_p(v.ctypes.data)
    rc = lib.dpq_flat_open_u8(ptr, n, D, device, id_offset, None if out is None else ctypes.byref(h))
    return rc, h


def test_flat_open_u8_argument_errors_come_before_any_device_call(lib):
    from deltapq_amd import api
    v = np.zeros((4, 8), dtype=np.uint8)
    assert _open_raw(lib, None, 4, 8)[0] == -1
    assert _open_raw(lib, v, 4, 8, out=None)[0] == -1
    assert _open_raw(lib, v, 0, 8)[0] == -1
    assert _open_raw(lib, v, 4, 0)[0] == -1
    assert _open_raw(lib, v, 4, 2049)[0] == -1
    assert _open_raw(lib, v, 4, 8, id_offset=-1)[0] == -1
    assert _open_raw(lib, v, 4, 8, id_offset=2 ** 31 - 4)[0] == -1        # n + id_offset == 2^31
    assert b"dpq_flat_open_u8" in lib.dpq_last_error()
    if api.device_count() == 0:                                            # ... and only then the device
        assert _open_raw(lib, v, 4, 8)[0] == -4
        with pytest.raises(api.DpqError) as e:
            api.FlatIndexU8(v)
        assert e.value.status == -4 and "no CPU fallback" in str(e.value)
    assert _open_raw(lib, v, 4, 8, device=10 ** 6)[0] == -4


def test_read_bvecs_range_equals_slices_of_read_vecs(lib, tmp_path):
    from deltapq_amd import api, synth
    rng = np.random.default_rng(3)
    n, D = 37, 10
    v = rng.integers(0, 256, size=(n, D)).astype(np.uint8)
    v[0, :4] = (0, 127, 128, 255)
    path = str(tmp_path / "v.bvecs")
    synth.write_bvecs(path, v.astype(np.float32))
    whole = api.read_vecs(path, "bvecs")                    # dpq_read_vecs(..., is_bvecs = 1): the bytes widened
    assert np.array_equal(whole.astype(np.uint8), v) and np.array_equal(whole, v.astype(np.float32))
    for first, count in ((0, n), (0, 1), (5, 20), (n - 1, 1), (n, 0), (12, 0)):
        got = api.read_bvecs_range(path, first, count)
        assert got.dtype == np.uint8 and got.shape == (count, D)
        assert np.array_equal(got, whole[first:first + count].astype(np.uint8))
    for first, count in ((0, n + 1), (n, 1), (30, 8)):
        with pytest.raises(api.DpqError) as e:
            api.read_bvecs_range(path, first, count)
        assert e.value.status == -2
    with pytest.raises(api.DpqError) as e:
        api.read_bvecs_range(str(tmp_path / "absent"), 0, 1)
    assert e.value.status == -2


def test_flat_index_u8_refuses_other_types_without_touching_the_library(monkeypatch):
    from deltapq_amd import _lib, api

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in (np.zeros((4, 8), dtype=np.float32), np.zeros((4, 8), dtype=np.int8), [[1, 2], [3, 4]]):
        with pytest.raises(TypeError):
            api.FlatIndexU8(bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
def test_gpu_asymmetric_rows_and_columns(gpu):
    """The first thing to run: a transposed or mis-mapped MFMA tile cannot pass."""
    i, j, d = np.arange(100)[:, None], np.arange(70)[:, None], np.arange(64)[None, :]
    base = ((7 * i + 3 * d) % 251).astype(np.uint8)
    qs = ((13 * j + 5 * d + 1) % 241).astype(np.uint8)
    with gpu.FlatIndexU8(base) as f:
        assert_same(f.search(qs, 100), U.search(base, qs, 100), "asymmetric rows and columns")


@pytest.mark.gpu
def test_gpu_rounding_pair_is_ordered_by_id(gpu):
    base, zero = rounding_pair()
    want = int(np.float32(16841476).view(np.uint32))
    with gpu.FlatIndexU8(base) as f:
        ids, d = f.search(zero, 8)
        assert ids[0, :2].tolist() == [3, 5] and bits(d)[0, :2].tolist() == [want, want]
        assert_same((ids, d), U.search(base, zero, 8), "rounding pair")
        ids, d = f.rerank(zero, np.array([[5, 3]], dtype=np.int32), 2)
        assert ids.tolist() == [[3, 5]] and bits(d).tolist() == [[want, want]]


@pytest.mark.gpu
@pytest.mark.parametrize("D,n,nq,top_k", [(1, 4099, 1, 1), (3, 4099, 65, 2048), (100, 4099, 3, 100), (130, 4099, 3, 100),
                                          (2048, 1031, 2, 1031)])
def test_gpu_sign_and_bias(gpu, D, n, nq, top_k):
    rng = np.random.default_rng(D * 7 + nq)
    values = np.array([0, 127, 128, 255], dtype=np.uint8)
    base = values[rng.integers(0, 4, size=(n, D))]
    qs = values[rng.integers(0, 4, size=(nq, D))]
    if D == 2048:                       # the largest distance there is: 2048 * 255^2 = 133 171 200, just below 2^27
        base[7], qs[0] = 255, 0
    want = U.search(base, qs, top_k)
    if D == 2048:
        assert want[1].max() == np.float32(2048 * 65025) and want[1].min() > 2.0 ** 24
    with gpu.FlatIndexU8(base) as f:
        assert_same(f.search(qs, top_k), want, "D %d n %d nq %d top-%d" % (D, n, nq, top_k))
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
def test_gpu_exact_ties(gpu):
    rng = np.random.default_rng(11)
    base = rng.integers(0, 6, size=(5000, 128)).astype(np.uint8)
    base[1000:2000] = base[0:1000]
    qs = (base[[3, 500, 999, 4000]] + rng.integers(0, 2, size=(4, 128))).astype(np.uint8)
    want = U.search(base, qs, 50)
    tied = sum(int((np.diff(bits(row)) == 0).sum()) for row in want[1])
    print("exactly tied neighbours in the restatement's lists:", tied)
    assert tied >= 3       # the copied rows tie pairwise
    with gpu.FlatIndexU8(base) as f:
        assert_same(f.search(qs, 50), want, "byte data with ties")


@pytest.mark.gpu
def test_gpu_every_stripe_lowers_the_threshold(gpu):
    """The base in descending distance to the first query: every vector beats the threshold so far.  40 000 rows are ten
    stripes at the smallest key capacity (8192 keys, stripes of 4096 rows)."""
    rng = np.random.default_rng(13)
    base = rng.integers(0, 256, size=(40000, 16)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(3, 16)).astype(np.uint8)
    base = base[np.argsort(-U.distances(base, qs[0]), kind="stable")]
    with gpu.FlatIndexU8(base) as f:
        assert_same(f.search(qs, 100), U.search(base, qs, 100), "descending order")


@pytest.mark.gpu
def test_gpu_offsets_and_parts(gpu):
    rng = np.random.default_rng(14)
    base = rng.integers(0, 4, size=(6000, 24)).astype(np.uint8)      # many ties across the cut
    qs = rng.integers(0, 4, size=(9, 24)).astype(np.uint8)
    k, cut = 300, 2500
    with gpu.FlatIndexU8(base, id_offset=1000) as f:
        whole = f.search(qs, k)
    assert_same(whole, U.search(base, qs, k, id_offset=1000), "id_offset")
    with gpu.FlatIndexU8(base[:cut], id_offset=1000) as a, gpu.FlatIndexU8(base[cut:], id_offset=1000 + cut) as b:
        ia, da = a.search(qs, k)
        ib, db = b.search(qs, k)
    assert_same(gpu.merge_topk_host(np.stack([ia, ib]), np.stack([da, db])), whole, "two parts merged")


@pytest.mark.gpu
def test_gpu_same_bits_as_the_fp32_path(gpu):
    rng = np.random.default_rng(15)
    base = rng.integers(0, 256, size=(8192, 128)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(64, 128)).astype(np.uint8)
    with gpu.FlatIndexU8(base) as f8, gpu.FlatIndex(base.astype(np.float32)) as f32:
        assert_same(f8.search(qs, 100), f32.search(qs.astype(np.float32), 100), "bytes against the widened fp32 search")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand,top_k,D", [(1, 1, 128), (100, 7, 100), (2048, 100, 128), (16384, 1000, 32)])
def test_gpu_rerank_matches_the_restatement(gpu, n_cand, top_k, D):
    import torch
    rng = np.random.default_rng(n_cand + top_k)
    n, nq, off = 5000, 7, 300
    base = rng.integers(0, 256, size=(n, D)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(nq, D)).astype(np.uint8)
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)     # with n_cand >= 100: duplicates
    cand[rng.random(size=cand.shape) < 0.2] = -1                               # padding
    if n_cand >= 100:
        cand[1, 5:] = -1                                                       # fewer valid candidates than top_k
        cand[2, :] = -1                                                        # none at all
        cand[3, :50] = cand[3, 50]
    with gpu.FlatIndexU8(base, id_offset=off) as f:
        want = U.rerank(base, qs, cand, top_k, id_offset=off)
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
        with pytest.raises(TypeError):
            f.rerank(qs.astype(np.float32), cand, top_k)


@pytest.mark.gpu
def test_gpu_rerank_with_a_map_and_the_even_n_rule(gpu):
    rng = np.random.default_rng(16)
    n, n_map, D, nq, n_cand, k = 3000, 2000, 64, 5, 300, 40
    base = rng.integers(0, 256, size=(n, D)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(nq, D)).astype(np.uint8)
    id_map = rng.permutation(n)[:n_map].astype(np.uint32)
    cand = rng.integers(0, n_map - 1, size=(nq, n_cand)).astype(np.int32)      # position n_map - 1 only through the rule
    cand[:, 7] = n_map                                                         # the even-N id of the last position
    cand[0, 8] = -1
    with gpu.FlatIndexU8(base, id_offset=50) as f:
        f.set_id_map(id_map)
        assert_same(f.rerank(qs, cand, k), U.rerank(base, qs, cand, k, id_offset=50, id_map=id_map), "rerank through a map")
        only = np.full((nq, 2), n_map, dtype=np.int32)
        ids, _ = f.rerank(qs, only, 1)
        assert (ids[:, 0] == int(id_map[n_map - 1]) + 50).all()
        bad = cand.copy()
        bad[2, 3] = n_map + 1
        with pytest.raises(gpu.DpqError) as e:
            f.rerank(qs, bad, k)
        assert e.value.status == -1
    with gpu.FlatIndexU8(base) as f:                                           # an odd map: n_map itself names nothing
        f.set_id_map(id_map[:n_map - 1])
        with pytest.raises(gpu.DpqError) as e:
            f.rerank(qs, np.full((nq, 2), n_map - 1, dtype=np.int32), 1)
        assert e.value.status == -1


@pytest.mark.gpu
def test_gpu_handle_kinds_do_not_mix(gpu, lib):
    b = np.zeros((16, 8), dtype=np.uint8)
    q8, q32 = np.zeros((1, 8), dtype=np.uint8), np.zeros((1, 8), dtype=np.float32)
    ids, d = np.empty((1, 1), dtype=np.int32), np.empty((1, 1), dtype=np.float32)
    cand = np.zeros((1, 1), dtype=np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    with gpu.FlatIndexU8(b) as f8, gpu.FlatIndex(b.astype(np.float32)) as f32:
        assert lib.dpq_flat_search(f8._h, p(q32), 1, 1, p(ids), p(d)) == -1
        assert b"dpq_flat_search_u8" in lib.dpq_last_error()
        assert lib.dpq_flat_rerank(f8._h, p(q32), 1, p(cand), 1, 1, p(ids), p(d)) == -1
        assert b"dpq_flat_rerank_u8" in lib.dpq_last_error()
        assert lib.dpq_flat_search_u8(f32._h, p(q8), 1, 1, p(ids), p(d)) == -1
        assert b"call dpq_flat_search" in lib.dpq_last_error()
        assert lib.dpq_flat_rerank_u8(f32._h, p(q8), 1, p(cand), 1, 1, p(ids), p(d)) == -1
        assert f8.search(q8, 1)[0].tolist() == [[0]] and f32.search(q32, 1)[0].tolist() == [[0]]   # both still work


@pytest.mark.gpu
def test_gpu_cli_groundtruth_over_bvecs(gpu, tmp_path):
    from deltapq_amd import synth
    rng = np.random.default_rng(17)
    d, n, nq, k = str(tmp_path), 3000, 5, 10
    base = rng.integers(0, 256, size=(n, 24)).astype(np.uint8)
    qs = rng.integers(0, 256, size=(nq, 24)).astype(np.uint8)
    synth.write_bvecs(os.path.join(d, "base.bvecs"), base.astype(np.float32))
    synth.write_bvecs(os.path.join(d, "query.bvecs"), qs.astype(np.float32))
    r = subprocess.run([EXE, "-dataset", d, "-task", "groundtruth", "-ext", "bvecs", "-topk", str(k), "-query_size", str(nq)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    gt_path = os.path.join(d, "groundtruth", "N%dTop%d.txt" % (n, k))
    assert gt_path in r.stdout
    assert_same(gpu.read_groundtruth(gt_path), U.search(base, qs, k), "ground-truth file over .bvecs")
