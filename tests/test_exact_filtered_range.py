"""Exact filtered and range search over raw vectors (dpq_flat_filter_*, dpq_flat_search_filtered*, dpq_flat_range_search*,
include/deltapq_amd.h).  The rules are restated in _exact_filter_range_restatement.py; the GPU is held to them on ids and
on distance bits -- the order (distance, id) is total, so nothing is left out and no tolerance exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _exact_filter_range_restatement as R
import _exact_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pack(mask):
    from deltapq_amd import api
    return api.IdFilter.pack_mask(mask)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_restatement_known_answers():
    """The five-row base of test_restatement_orders_by_distance_then_id: distances 4, 1, 1, 9, 1 for ids 10 .. 14."""
    base = np.array([[2.0], [1.0], [-1.0], [3.0], [1.0]], dtype=np.float32)
    q = np.zeros((1, 1), dtype=np.float32)
    mask = np.ones(15, dtype=bool)
    mask[11] = False                                                       # the filter removes id 11
    w, nb = pack(mask)
    ids, d = R.search_filtered(base, q, 4, w, nb, id_offset=10)
    assert ids.tolist() == [[12, 14, 10, 13]] and d.tolist() == [[1.0, 1.0, 4.0, 9.0]]
    ids, d = R.search_filtered(base, q, 6, w, nb, id_offset=10)
    assert ids.tolist() == [[12, 14, 10, 13, -1, -1]] and d.tolist() == [[1.0, 1.0, 4.0, 9.0, np.inf, np.inf]]
    ids, d = R.search_filtered(base, q, 2, w, 12, id_offset=10)             # a bitmap of 12 bits: ids 10 and (cleared) 11
    assert ids.tolist() == [[10, -1]] and d.tolist() == [[4.0, np.inf]]
    lims, ids, d = R.range_search(base, q, 1.0, id_offset=10)              # strictly below 1.0: nothing
    assert lims.tolist() == [0, 0] and ids.size == 0 and d.size == 0
    lims, ids, d = R.range_search(base, q, np.nextafter(np.float32(1.0), np.float32(2.0)), id_offset=10)
    assert lims.tolist() == [0, 3] and ids.tolist() == [11, 12, 14] and d.tolist() == [1.0, 1.0, 1.0]
    lims, ids, d = R.range_search(base, q, np.nextafter(np.float32(1.0), np.float32(2.0)), w, nb, id_offset=10)
    assert lims.tolist() == [0, 2] and ids.tolist() == [12, 14]
    lims, ids, d = R.range_search(base, np.zeros((3, 1), dtype=np.float32), [np.inf, 0.0, -1.0], w, nb, id_offset=10)
    assert lims.tolist() == [0, 4, 4, 4] and ids.tolist() == [12, 14, 10, 13] and d.tolist() == [1.0, 1.0, 4.0, 9.0]
    vec_id = np.array([2, 0, 3, 1], dtype=np.uint32)                        # even N: position 3 is reported as 4
    w, nb = pack(np.array([True, True, False, False]))                     # vectors 0 and 1
    assert R.bitmap_to_dfs(w, nb, vec_id).tolist() == [0b10010]


def test_argument_errors_come_before_any_device_call(lib):
    """Every check that needs no handle runs first, then the device, then the handle: a made-up handle is never read."""
    from deltapq_amd import api
    fake, fake_f = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    out = ctypes.c_void_p()
    w = np.ones(1, dtype=np.uint32)
    q = np.zeros((2, 4), dtype=np.float32)
    q8 = np.zeros((2, 4), dtype=np.uint8)
    ids = np.zeros((2, 3), dtype=np.int32)
    d = np.zeros((2, 3), dtype=np.float32)
    rad = np.ones(2, dtype=np.float32)
    nan = np.array([1.0, np.nan], dtype=np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731

    def err(rc, name):
        assert rc == -1, (name, rc)
        assert name.encode() in lib.dpq_last_error(), lib.dpq_last_error()

    err(lib.dpq_flat_filter_create(fake, p(w), 8, None), "dpq_flat_filter_create")
    err(lib.dpq_flat_filter_create(None, p(w), 8, out), "dpq_flat_filter_create")
    err(lib.dpq_flat_filter_create(fake, p(w), -1, out), "dpq_flat_filter_create")
    err(lib.dpq_flat_filter_create(fake, None, 8, out), "dpq_flat_filter_create")
    lib.dpq_flat_filter_free(None)                                          # nothing happens
    n = ctypes.c_int64()
    err(lib.dpq_flat_filter_count(None, n), "dpq_flat_filter_count")
    for fn, name, qq in ((lib.dpq_flat_search_filtered, "dpq_flat_search_filtered", q),
                         (lib.dpq_flat_search_filtered_u8, "dpq_flat_search_filtered_u8", q8)):
        err(fn(None, fake_f, p(qq), 2, 3, p(ids), p(d)), name)
        err(fn(fake, None, p(qq), 2, 3, p(ids), p(d)), name)                # a NULL filter
        err(fn(fake, fake_f, None, 2, 3, p(ids), p(d)), name)
        err(fn(fake, fake_f, p(qq), 2, 3, None, p(d)), name)
        err(fn(fake, fake_f, p(qq), 2, 3, p(ids), None), name)
        err(fn(fake, fake_f, p(qq), -1, 3, p(ids), p(d)), name)
        err(fn(fake, fake_f, p(qq), 2, 0, p(ids), p(d)), name)
        err(fn(fake, fake_f, p(qq), 2, 16385, p(ids), p(d)), name)
    for fn, name, qq in ((lib.dpq_flat_range_search, "dpq_flat_range_search", q),
                         (lib.dpq_flat_range_search_u8, "dpq_flat_range_search_u8", q8)):
        err(fn(fake, None, p(qq), 2, p(rad), None), name)
        err(fn(None, None, p(qq), 2, p(rad), out), name)
        err(fn(fake, None, None, 2, p(rad), out), name)
        err(fn(fake, None, p(qq), 2, None, out), name)
        err(fn(fake, None, p(qq), -1, p(rad), out), name)
        err(fn(fake, None, p(qq), 2, p(nan), out), name)
        assert b"NaN" in lib.dpq_last_error() and out.value is None
    if api.device_count() == 0:                                             # ... and only then the device
        assert lib.dpq_flat_filter_create(fake, p(w), 8, out) == -4
        assert b"dpq_flat_filter_create" in lib.dpq_last_error()
        assert lib.dpq_flat_search_filtered(fake, fake_f, p(q), 2, 3, p(ids), p(d)) == -4
        assert lib.dpq_flat_search_filtered_u8(fake, fake_f, p(q8), 2, 3, p(ids), p(d)) == -4
        assert lib.dpq_flat_range_search(fake, None, p(q), 2, p(rad), out) == -4
        assert lib.dpq_flat_range_search_u8(fake, fake_f, p(q8), 2, p(rad), out) == -4
        assert b"dpq_flat_range_search_u8" in lib.dpq_last_error() and b"no CPU fallback" in lib.dpq_last_error()


def test_range_recall_on_hand_written_lists(lib):
    from deltapq_amd import api
    L = lambda *a: np.array(a, dtype=np.int64)     # noqa: E731
    I = lambda *a: np.array(a, dtype=np.int32)     # noqa: E731
    # q0: found {1, 2, 3} truth {2, 3, 4, 5} -> 2 hits; q1: found {7} truth {} ; q2: found {} truth {9}
    found = (L(0, 3, 4, 4), I(1, 2, 3, 7))
    truth = (L(0, 4, 4, 5), I(2, 3, 4, 5, 9))
    assert api.range_recall(found, truth) == (2 / 5, 2 / 4)
    assert R.range_recall(found, truth) == (2 / 5, 2 / 4)
    # a repeated id counts once, a negative id not at all
    found = (L(0, 5), I(4, 4, -1, 6, 4))
    truth = (L(0, 4), I(4, -1, 5, 5))
    assert api.range_recall(found, truth) == (1 / 2, 1 / 2)
    assert R.range_recall(found, truth) == (1 / 2, 1 / 2)
    empty = (L(0, 0), I())
    assert api.range_recall(empty, empty) == (1.0, 1.0)                      # both denominators zero
    assert api.range_recall(empty, (L(0, 2), I(1, 2))) == (0.0, 1.0)         # empty found: precision 1
    assert api.range_recall((L(0, 2), I(1, 2)), empty) == (1.0, 0.0)         # empty truth: recall 1
    rec = ctypes.c_double(-1)
    fl, fi = L(0, 1), I(3)
    assert lib.dpq_range_recall(1, fl.ctypes.data, fi.ctypes.data, fl.ctypes.data, fi.ctypes.data, rec, None) == 0
    assert rec.value == 1.0                                                  # either output may be NULL
    assert lib.dpq_range_recall(1, fl.ctypes.data, fi.ctypes.data, fl.ctypes.data, fi.ctypes.data, None, rec) == 0
    assert lib.dpq_range_recall(1, None, fi.ctypes.data, fl.ctypes.data, fi.ctypes.data, rec, rec) == -1
    assert lib.dpq_range_recall(-1, fl.ctypes.data, fi.ctypes.data, fl.ctypes.data, fi.ctypes.data, rec, rec) == -1


def test_bitmap_to_dfs_on_hand_written_vec_id(lib):
    from deltapq_amd import api
    # odd N = 5: position p holds vector vec_id[p]; vectors 1 and 4 allowed -> positions 2 and 0
    vec_id = np.array([4, 0, 1, 3, 2], dtype=np.uint32)
    w, nb = pack(np.array([False, True, False, False, True]))
    out, out_bits = api.bitmap_to_dfs(w, nb, vec_id)
    assert out_bits == 6 and out.tolist() == [0b00101]
    assert R.bitmap_to_dfs(w, nb, vec_id).tolist() == [0b00101]
    # even N = 6: the last position (5, vector 2) is reported as 6: bit 6 governs it, bit 5 stays clear
    vec_id = np.array([4, 0, 1, 3, 5, 2], dtype=np.uint32)
    w, nb = pack(np.array([False, True, True, False, False, False]))
    out, out_bits = api.bitmap_to_dfs(w, nb, vec_id)
    assert out_bits == 7 and out.tolist() == [0b1000100]
    assert R.bitmap_to_dfs(w, nb, vec_id).tolist() == [0b1000100]
    w, nb = pack(np.ones(6, dtype=bool))
    assert api.bitmap_to_dfs(w, nb, vec_id)[0].tolist() == [0b1011111]
    # n_bits shorter than the largest vec_id: vectors 3, 4, 5 have no bit
    w, nb = pack(np.ones(3, dtype=bool))
    assert api.bitmap_to_dfs(w, nb, vec_id)[0].tolist() == [0b1000110]
    assert R.bitmap_to_dfs(w, nb, vec_id).tolist() == [0b1000110]
    assert api.bitmap_to_dfs(np.zeros(0, dtype=np.uint32), 0, vec_id)[0].tolist() == [0]
    # across a word boundary, against the restatement
    rng = np.random.default_rng(5)
    for n in (63, 64, 65, 200):
        vec_id = rng.permutation(n).astype(np.uint32)
        w, nb = pack(rng.random(n - 7) < 0.5)
        assert api.bitmap_to_dfs(w, nb, vec_id)[0].tolist() == R.bitmap_to_dfs(w, nb, vec_id).tolist()
    out = np.zeros(1, dtype=np.uint32)
    assert lib.dpq_bitmap_to_dfs(w.ctypes.data, nb, None, 5, out.ctypes.data) == -1
    assert lib.dpq_bitmap_to_dfs(w.ctypes.data, -1, vec_id.ctypes.data, 5, out.ctypes.data) == -1
    assert lib.dpq_bitmap_to_dfs(w.ctypes.data, nb, vec_id.ctypes.data, 5, None) == -1


def test_bitmap_file_round_trip_and_truncation(lib, tmp_path):
    from deltapq_amd import api
    rng = np.random.default_rng(6)
    for n in (0, 1, 32, 33, 1000):
        w, nb = pack(rng.random(n) < 0.5)
        path = str(tmp_path / ("f%d.bitmap" % n))
        api.write_bitmap(path, w, nb)
        assert os.path.getsize(path) == 8 + 4 * ((n + 31) // 32)
        raw = open(path, "rb").read()
        assert int.from_bytes(raw[:8], "little") == n and raw[8:] == w.astype("<u4").tobytes()
        w2, nb2 = api.read_bitmap(path)
        assert nb2 == nb and w2.tolist() == w.tolist()
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 1)
    with pytest.raises(api.DpqError) as e:
        api.read_bitmap(path)
    assert e.value.status == -2                                             # DPQ_ERR_IO
    with open(path, "r+b") as f:
        f.truncate(5)
    with pytest.raises(api.DpqError) as e:
        api.read_bitmap(path)
    assert e.value.status == -2
    with pytest.raises(api.DpqError) as e:
        api.read_bitmap(str(tmp_path / "absent"))
    assert e.value.status == -2


def test_cli_usage_names_the_filter_flag(built):
    r = subprocess.run([EXE, "-task", "groundtruth"], capture_output=True, text=True)
    assert r.returncode == 2 and "-filter FILE" in r.stdout
    r = subprocess.run([EXE, "-task", "recall"], capture_output=True, text=True)
    assert r.returncode == 2 and "-filter FILE" in r.stdout
    r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "recall", "-m", "8", "-k", "256", "-N", "10", "-query_size", "1",
                        "-topk", "1", "-rerank", "5", "-filter", "x"], capture_output=True, text=True)
    assert r.returncode == 1 and "-rerank cannot be combined with -filter" in r.stdout


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
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    bad_i = int((gi != wi).sum())
    bad_d = int((bits(gd) != bits(wd)).sum())
    if bad_i or bad_d:
        print("%s: %d of %d ids and %d of %d distance bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert bad_i == 0 and bad_d == 0, what


def assert_same_range(got, want, what):
    assert got[0].tolist() == want[0].tolist(), what + ": lims"
    assert_same(got[1:], want[1:], what)


NS = [1, 63, 64, 65, 255, 257, 4096, 4097, 9000]   # tile edges 64 / 256 and the 4096-entry stripe of top_k <= 2048
NQS = [1, 65]
TOPKS = [1, 10, 100]


def filters_for(n, rng):
    """name -> (words, n_bits) over ids 0 .. (id_offset = 0)."""
    block = np.zeros(n, dtype=bool)
    lo = 250 if n >= 262 else min(60, n - 1)
    block[lo:lo + 12] = True                                                # straddles row 256 (or 64)
    single = np.zeros(n, dtype=bool)
    single[n // 2] = True
    every64 = np.zeros(n, dtype=bool)
    every64[::64] = True
    return {
        "all": pack(np.ones(n, dtype=bool)),
        "none": pack(np.zeros(n, dtype=bool)),
        "no bits": (np.zeros(0, dtype=np.uint32), 0),
        "single": pack(single),
        "every 64th": pack(every64),
        "block": pack(block),
        "50 %": pack(rng.random(n) < 0.5),
        "1 %": pack(rng.random(n) < 0.01),
        "shorter": pack(np.ones(n // 2, dtype=bool)),
        "longer": pack(np.ones(n + 100, dtype=bool)),
    }


def run_filtered_shapes(gpu, index_cls, filter_base, base, qs, n, D):
    rng = np.random.default_rng(n * 31 + D)
    dist = R.all_distances(filter_base, qs)                                 # once per shape, shared and left unchanged
    with index_cls(base) as f:
        for name, (w, nb) in filters_for(n, rng).items():
            with gpu.FlatIdFilter(f, w, nb) as ff:
                assert ff.n_allowed == int(R.eligible(n, 0, w, nb).sum()), name
                for nq in NQS:
                    for k in TOPKS:
                        want = R.search_filtered(filter_base, qs[:nq], k, w, nb, dist=dist[:nq])
                        assert_same(f.search_filtered(qs[:nq], k, ff), want, "n %d D %d nq %d top-%d filter %s" % (n, D, nq, k, name))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3, 33])
@pytest.mark.parametrize("n", NS)
def test_gpu_filtered_search_fp32(gpu, n, D):
    rng = np.random.default_rng(n * 7 + D)
    base = rng.integers(-3, 4, size=(n, D)).astype(np.float32) + (rng.random((n, D)) < 0.3) * rng.normal(size=(n, D)).astype(np.float32)
    base = base.astype(np.float32)                                          # integer rows tie, the others do not
    qs = rng.integers(-3, 4, size=(65, D)).astype(np.float32)
    run_filtered_shapes(gpu, gpu.FlatIndex, base, base, qs, n, D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 31, 32, 33, 128])
@pytest.mark.parametrize("n", NS)
def test_gpu_filtered_search_u8(gpu, n, D):
    rng = np.random.default_rng(n * 11 + D)
    base = rng.integers(0, 256 if D > 1 else 40, size=(n, D), dtype=np.uint8)
    qs = rng.integers(0, 256 if D > 1 else 40, size=(65, D), dtype=np.uint8)
    dist = R.all_distances(base.astype(np.float32), qs.astype(np.float32))
    frng = np.random.default_rng(n * 31 + D)
    with gpu.FlatIndexU8(base) as f:
        for name, (w, nb) in filters_for(n, frng).items():
            with gpu.FlatIdFilter(f, w, nb) as ff:
                assert ff.n_allowed == int(R.eligible(n, 0, w, nb).sum()), name
                for nq in NQS:
                    for k in TOPKS:
                        want = R.search_filtered(base, qs[:nq], k, w, nb, dist=dist[:nq])
                        assert_same(f.search_filtered(qs[:nq], k, ff), want, "u8 n %d D %d nq %d top-%d filter %s" % (n, D, nq, k, name))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32", "u8"])
def test_gpu_fewer_eligible_rows_than_top_k(gpu, kind):
    rng = np.random.default_rng(21)
    n, D = 4097, 33
    base8 = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    qs8 = rng.integers(0, 256, size=(5, D), dtype=np.uint8)
    base, qs = base8.astype(np.float32), qs8.astype(np.float32)
    dist = R.all_distances(base, qs)
    with (gpu.FlatIndex(base) if kind == "fp32" else gpu.FlatIndexU8(base8)) as f:
        q = qs if kind == "fp32" else qs8
        for k in (1, 10, 100):
            for m in (0, k - 1, k):
                ids = rng.choice(n, size=m, replace=False)
                w, nb = gpu.IdFilter.pack_ids(ids, n)
                with gpu.FlatIdFilter.from_ids(f, ids, n) as ff:
                    assert ff.n_allowed == m
                    gi, gd = f.search_filtered(q, k, ff)
                assert_same((gi, gd), R.search_filtered(base, qs, k, w, nb, dist=dist), "%s: %d eligible, top-%d" % (kind, m, k))
                assert (gi[:, m:] == -1).all() and (bits(gd[:, m:]) == 0x7F800000).all()
                assert (gi[:, :m] >= 0).all() and all(sorted(row[:m].tolist()) == sorted(ids.tolist()) for row in gi)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32", "u8"])
def test_gpu_id_offset_parts_and_a_global_bitmap(gpu, kind):
    rng = np.random.default_rng(22)
    n, D, off, cut, k = 6001, 24, 1000, 3000, 50
    base8 = rng.integers(0, 4, size=(n, D), dtype=np.uint8)                 # many ties across the cut
    qs8 = rng.integers(0, 4, size=(9, D), dtype=np.uint8)
    base, qs = base8.astype(np.float32), qs8.astype(np.float32)
    mask = rng.random(off + n - 500) < 0.3                                  # ends 500 ids before the base does
    mask[:off] = True                                                       # bits below id_offset govern nothing
    w, nb = pack(mask)
    want = R.search_filtered(base, qs, k, w, nb, id_offset=off)
    assert want[0].min() >= off
    cls = gpu.FlatIndex if kind == "fp32" else gpu.FlatIndexU8
    b, q = (base, qs) if kind == "fp32" else (base8, qs8)
    with cls(b, id_offset=off) as f, gpu.FlatIdFilter(f, w, nb) as ff:
        assert_same(f.search_filtered(q, k, ff), want, "one handle, id_offset 1000")
        assert_same_range(f.range_search(q, 12.0, ff), R.range_search(base, qs, 12.0, w, nb, id_offset=off), "range, id_offset 1000")
    parts = []
    for r0, r1 in ((0, cut), (cut, n)):
        with cls(b[r0:r1], id_offset=off + r0) as f, gpu.FlatIdFilter(f, w, nb) as ff:
            parts.append(f.search_filtered(q, k, ff))
    merged = gpu.merge_topk_host(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert_same(merged, want, "two parts with their own filters, merged")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32", "u8"])
def test_gpu_duplicate_heavy_base_next_lowest_ids_win(gpu, kind):
    rng = np.random.default_rng(23)
    n, D, k = 4100, 16, 10
    protos = rng.integers(0, 256, size=(8, D), dtype=np.uint8)
    base8 = protos[np.arange(n) % 8]
    qs8 = protos[[0, 5]]
    mask = np.ones(n, dtype=bool)
    mask[[0, 8, 16, 5, 13]] = False                                         # the lowest ids of the two tie groups
    w, nb = pack(mask)
    cls = gpu.FlatIndex if kind == "fp32" else gpu.FlatIndexU8
    b, q = (base8.astype(np.float32), qs8.astype(np.float32)) if kind == "fp32" else (base8, qs8)
    with cls(b) as f, gpu.FlatIdFilter(f, w, nb) as ff:
        ids, d = f.search_filtered(q, k, ff)
    assert ids[0].tolist() == [24 + 8 * i for i in range(k)] and ids[1].tolist() == [21 + 8 * i for i in range(k)]
    assert (bits(d) == 0).all()
    assert_same((ids, d), R.search_filtered(base8, qs8, k, w, nb), "duplicate-heavy")


@pytest.mark.gpu
def test_gpu_all_ones_filter_equals_the_unfiltered_search(gpu):
    rng = np.random.default_rng(24)
    n, D = 9000, 33
    base8 = rng.integers(0, 6, size=(n, D), dtype=np.uint8)
    qs8 = rng.integers(0, 6, size=(65, D), dtype=np.uint8)
    for cls, b, q in ((gpu.FlatIndex, base8.astype(np.float32), qs8.astype(np.float32)), (gpu.FlatIndexU8, base8, qs8)):
        with cls(b) as f, gpu.FlatIdFilter.from_mask(f, np.ones(n, dtype=bool)) as ff:
            for k in (1, 100, 3000):
                a, c = f.search(q, k), f.search_filtered(q, k, ff)
                assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes(), (cls.__name__, k)
            # range search: the direct-row kernels (no filter) against the list kernels (the all-ones filter)
            for radius in (np.inf, f.search(q, 10)[1][:, 9].copy()):
                a, c = f.range_search(q, radius), f.range_search(q, radius, ff)
                assert len(a) == 3 and len(c) == 3
                for x, y, what in zip(a, c, ("lims", "ids", "dists")):
                    assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (cls.__name__, what)
            assert a[0][-1] > 0  # the last radius, every query's 10th distance, lets rows in


@pytest.mark.gpu
def test_gpu_filtered_kernel_keeps_the_in_order_sum(gpu):
    import test_exact_search as T
    v = T.order_vector()
    base = np.stack([np.zeros(514, dtype=np.float32), v, v[::-1]])
    q = np.zeros((1, 514), dtype=np.float32)
    with gpu.FlatIndex(base) as f, gpu.FlatIdFilter.from_ids(f, [1], 3) as ff:
        ids, d = f.search_filtered(q, 2, ff)
        assert ids.tolist() == [[1, -1]] and bits(d).tolist() == [[0x3F800000, 0x7F800000]]
        lims, ids, d = f.range_search(q, np.inf, ff)
        assert lims.tolist() == [0, 1] and ids.tolist() == [1] and bits(d).tolist() == [0x3F800000]
        lims, ids, d = f.range_search(q, np.inf)
        assert ids.tolist() == [0, 1, 2] and bits(d).tolist() == [0, 0x3F800000, 0x3F800001]


@pytest.mark.gpu
def test_gpu_byte_handle_equals_fp32_handle_on_the_widened_data(gpu):
    rng = np.random.default_rng(25)
    n, D = 4097, 33
    base8 = rng.integers(0, 256, size=(n, D), dtype=np.uint8)
    qs8 = rng.integers(0, 256, size=(65, D), dtype=np.uint8)
    w, nb = pack(rng.random(n) < 0.5)
    with gpu.FlatIndex(base8.astype(np.float32)) as f, gpu.FlatIdFilter(f, w, nb) as ff, \
            gpu.FlatIndexU8(base8) as f8, gpu.FlatIdFilter(f8, w, nb) as ff8:
        q = qs8.astype(np.float32)
        truth = f.search(q, 10)
        r = truth[1][:, 9].copy()
        assert_same(f8.search_filtered(qs8, 100, ff8), f.search_filtered(q, 100, ff), "filtered, bytes against fp32")
        assert_same_range(f8.range_search(qs8, r), f.range_search(q, r), "range, bytes against fp32")
        assert_same_range(f8.range_search(qs8, r * 2, ff8), f.range_search(q, r * 2, ff), "filtered range, bytes against fp32")


def tenth_distance(dist, mask):
    """Per query the 10th smallest distance among the eligible rows (the largest, with fewer than 10; 1.0 with none)."""
    out = np.ones(dist.shape[0], dtype=np.float32)
    rows = np.flatnonzero(mask)
    if len(rows):
        s = np.sort(dist[:, rows], axis=1)
        out = s[:, min(9, len(rows) - 1)].copy()
    return out


def run_range_shapes(gpu, f, q, base, qs, n, what):
    """f: the opened handle, q its queries; base / qs the fp32 view of the same data."""
    rng = np.random.default_rng(n)
    dist = R.all_distances(base, qs)
    nq = len(qs)
    w, nb = pack(rng.random(n) < 0.5)
    with gpu.FlatIdFilter(f, w, nb) as ff:
        for filt, fw, fb in ((None, None, 0), (ff, w, nb)):
            r10 = tenth_distance(dist, R.eligible(n, 0, fw, fb))
            mixed = np.array([[0.0, -1.0, np.inf][i % 3] for i in range(nq)], dtype=np.float32)
            for name, radii in (("0", np.zeros(nq, dtype=np.float32)), ("negative", np.full(nq, -2.5, dtype=np.float32)),
                                ("+inf", np.full(nq, np.inf, dtype=np.float32)), ("the 10th distance", r10),
                                ("nextafter the 10th distance", np.nextafter(r10, INF)), ("0 / negative / +inf by query", mixed)):
                want = R.range_search(base, qs, radii, fw, fb, dist=dist)
                got = f.range_search(q, radii, filt)
                assert_same_range(got, want, "%s n %d radius %s filter %s" % (what, n, name, filt is not None))
                if name == "the 10th distance" and fw is None and n >= 10:
                    assert (np.diff(want[0]) <= 9).all()                    # strictly below the 10th: at most nine
                if name == "nextafter the 10th distance" and fw is None and n >= 10:
                    assert (np.diff(want[0]) >= 10).all()                   # ties at the 10th distance included


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3, 33])
@pytest.mark.parametrize("n", NS)
def test_gpu_range_search_fp32(gpu, n, D):
    """n = 9000 with +inf: 65 lists of 9000 entries, 585 000 keys -- more than the 2^19 keys of a sub-batch's pool."""
    rng = np.random.default_rng(n * 13 + D)
    base = rng.integers(-3, 4, size=(n, D)).astype(np.float32)
    base[::3] += rng.normal(size=(len(base[::3]), D)).astype(np.float32)
    qs = rng.integers(-3, 4, size=(65, D)).astype(np.float32)
    with gpu.FlatIndex(base) as f:
        run_range_shapes(gpu, f, qs, base, qs, n, "fp32 D %d" % D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 31, 32, 33, 128])
@pytest.mark.parametrize("n", NS)
def test_gpu_range_search_u8(gpu, n, D):
    rng = np.random.default_rng(n * 17 + D)
    base8 = rng.integers(0, 256 if D > 1 else 40, size=(n, D), dtype=np.uint8)
    qs8 = rng.integers(0, 256 if D > 1 else 40, size=(65, D), dtype=np.uint8)
    with gpu.FlatIndexU8(base8) as f:
        run_range_shapes(gpu, f, qs8, base8.astype(np.float32), qs8.astype(np.float32), n, "u8 D %d" % D)


@pytest.mark.gpu
def test_gpu_range_search_more_queries_than_one_counting_pass(gpu):
    """1030 queries: the lists are counted 1024 queries at a time."""
    rng = np.random.default_rng(26)
    n, nq = 65, 1030
    base = rng.integers(0, 50, size=(n, 1)).astype(np.float32)
    qs = rng.integers(0, 50, size=(nq, 1)).astype(np.float32)
    radii = rng.integers(0, 30, size=nq).astype(np.float32)
    with gpu.FlatIndex(base) as f:
        assert_same_range(f.range_search(qs, radii), R.range_search(base, qs, radii), "1030 queries")
        lims, ids, d = f.range_search(qs[:0], 1.0)                           # nq == 0
        assert lims.tolist() == [0] and ids.size == 0


@pytest.mark.gpu
def test_gpu_foreign_filters_and_mixed_handle_kinds_are_refused(gpu, lib):
    base8 = np.arange(40, dtype=np.uint8).reshape(10, 4)
    q8 = base8[:2].copy()
    q = q8.astype(np.float32)
    w, nb = pack(np.ones(10, dtype=bool))
    ids = np.zeros((2, 3), dtype=np.int32)
    d = np.zeros((2, 3), dtype=np.float32)
    rad = np.ones(2, dtype=np.float32)
    out = ctypes.c_void_p()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    with gpu.FlatIndex(base8.astype(np.float32)) as f, gpu.FlatIndex(base8.astype(np.float32)) as g, gpu.FlatIndexU8(base8) as f8, \
            gpu.FlatIdFilter(f, w, nb) as ff, gpu.FlatIdFilter(f8, w, nb) as ff8:
        for call in (lambda: g.search_filtered(q, 3, ff), lambda: g.range_search(q, 1.0, ff),
                     lambda: f.search_filtered(q, 3, ff8), lambda: f8.range_search(q8, 1.0, ff)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == -1 and "another handle" in str(e.value)
        # an fp32 call on a byte handle and the reverse: DPQ_ERR_ARG naming the other function
        assert lib.dpq_flat_search_filtered(f8._h, ff8._h, p(q), 2, 3, p(ids), p(d)) == -1
        assert b"dpq_flat_search_filtered_u8" in lib.dpq_last_error()
        assert lib.dpq_flat_search_filtered_u8(f._h, ff._h, p(q8), 2, 3, p(ids), p(d)) == -1
        assert b"call dpq_flat_search_filtered" in lib.dpq_last_error()
        assert lib.dpq_flat_range_search(f8._h, None, p(q), 2, p(rad), out) == -1
        assert b"dpq_flat_range_search_u8" in lib.dpq_last_error() and out.value is None
        assert lib.dpq_flat_range_search_u8(f._h, None, p(q8), 2, p(rad), out) == -1
        assert b"call dpq_flat_range_search" in lib.dpq_last_error()
        with pytest.raises(TypeError):
            f.search_filtered(q, 3, None)
        for bad in (0, 16385):
            with pytest.raises(gpu.DpqError) as e:
                f.search_filtered(q, bad, ff)
            assert e.value.status == -1
        gi, gd = f.search_filtered(q[:0], 3, ff)                             # nq == 0
        assert gi.shape == (0, 3)
        gi, gd = f.search_filtered(q, 12, ff)                                # top_k above n: padding, no DPQ_ERR_TOPK
        assert (gi[:, 10:] == -1).all() and (gi[:, :10] >= 0).all()


def _positions_to_ids(pos, vec_id):
    n = len(vec_id)
    p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    return np.where(pos < 0, -1, vec_id[np.clip(p, 0, n - 1)].astype(np.int64)).astype(np.int32)


@pytest.mark.gpu
def test_gpu_cli_filtered_groundtruth_and_recall(gpu, tmp_path):
    from deltapq_amd import synth
    d, n, nq, k = str(tmp_path), 2000, 8, 20
    learn = synth.make_clustered_vectors(3000, 128, seed=81, n_clusters=60, centre_seed=80)
    base = synth.make_clustered_vectors(n, 128, seed=82, n_clusters=60, centre_seed=80)
    qs = synth.make_clustered_vectors(nq, 128, seed=83, n_clusters=60, centre_seed=80)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), learn)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), qs)
    w, nb = pack(np.random.default_rng(84).random(n - 100) < 0.25)           # the last 100 vectors have no bit
    fpath = os.path.join(d, "quarter.bitmap")
    gpu.write_bitmap(fpath, w, nb)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    env = dict(os.environ, DPQ_DEV="1", DPQ_GT_PART_ROWS="700")              # three parts of the base
    gt = ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)]
    rec = ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k)]
    outs = {}
    for name, args in (("learn", ["-task", "learn"]), ("encode", ["-task", "encode"]),
                       ("tree", ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"]),
                       ("gt", gt), ("gt_f", gt + ["-filter", fpath]), ("rec", rec), ("rec_f", rec + ["-filter", fpath])):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300, env=env if name.startswith("gt") else None)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr    # a failed step ends the chain
        outs[name] = r.stdout
    plain_path = os.path.join(d, "groundtruth", "N%dTop%d.txt" % (n, k))
    filt_path = os.path.join(d, "groundtruth", "N%dTop%d.filtered.txt" % (n, k))
    for o, path in ((outs["gt"], plain_path), (outs["gt_f"], filt_path)):
        assert "%d base vectors in 3 part(s)" % n in o and o.rstrip().endswith(path), o
    assert_same(gpu.read_groundtruth(filt_path), R.search_filtered(base, qs, k, w, nb), "filtered ground-truth file")
    truth = gpu.read_groundtruth(plain_path)
    assert_same(truth, X.search(base, qs, k), "ground-truth file without -filter")
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    n_codes, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n), n)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        pos, _ = idx.query_batch(qs, k)
        with gpu.IdFilter(idx, *gpu.bitmap_to_dfs(w, nb, vec_id)) as filt:
            pos_f, _ = idx.query_batch_filtered(qs, k, filt)
    found_f = _positions_to_ids(pos_f, vec_id)
    allowed = R.eligible(n, 0, w, nb)
    assert allowed[found_f[found_f >= 0]].all()                              # the translated bitmap allows what the file does
    want = X.recall(_positions_to_ids(pos, vec_id), truth[0], k, k)
    want_f = X.recall(found_f, gpu.read_groundtruth(filt_path)[0], k, k)
    got = re.search(r"^recall@%d = ([0-9.]+)$" % k, outs["rec"], re.M)
    got_f = re.search(r"^filtered recall@%d = ([0-9.]+)$" % k, outs["rec_f"], re.M)
    assert got and got_f, outs["rec"] + outs["rec_f"]
    print("CLI:", got.group(0), "|", got_f.group(0), "| restatement: %.6f %.6f" % (want, want_f))
    assert got.group(1) == "%.6f" % want and got_f.group(1) == "%.6f" % want_f
    assert "filtered recall" not in outs["rec"] and ".filtered.txt" not in outs["gt"]
