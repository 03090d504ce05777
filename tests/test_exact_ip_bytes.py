"""Exact inner product over byte vectors and signed int8 storage (dpq_flat_*_ip_u8, dpq_flat_open_i8, dpq_flat_*_i8,
dpq_flat_*_ip_i8; include/deltapq_amd.h).  The rules are restated in _exact_bytes_ip_restatement.py; the GPU is held to them
bit for bit on ids and on float bits -- every answer is an integer below 2^31, the order is total, no tie slack."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _exact_bytes_ip_restatement as B
import _exact_ip_restatement as XI
import _exact_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")

DTYPE = {"u8": np.uint8, "i8": np.int8}
# (kind of handle, metric) of the new calls; u8 by L2 is test_exact_search_u8.py's ground
COMBOS = [("u8", "ip"), ("i8", "l2"), ("i8", "ip")]
SUFFIX = {("u8", "l2"): "_u8", ("u8", "ip"): "_ip_u8", ("i8", "l2"): "_i8", ("i8", "ip"): "_ip_i8", ("f32", "l2"): "", ("f32", "ip"): "_ip"}
SHAPES = [("search", ""), ("search_filtered", ""), ("range_search", ""), ("rerank", ""), ("rerank", "_device")]


def fn_name(shape, tail, kind, metric):
    return "dpq_flat_%s%s%s" % (shape, SUFFIX[(kind, metric)], tail)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rand(rng, kind, shape):
    lo, hi = (0, 256) if kind == "u8" else (-128, 128)
    return rng.integers(lo, hi, size=shape).astype(DTYPE[kind])


def hand_case(kind):
    """(base, query, {metric: the integer answers}) of the contract's hand answers, D = 3."""
    if kind == "u8":
        return (np.array([[255, 255, 255], [0, 0, 0], [1, 2, 3]], dtype=np.uint8), np.full((1, 3), 255, dtype=np.uint8),
                {"ip": [195075, 0, 1530]})
    return (np.array([[-128, -128, -128], [127, 127, 127], [0, 0, 0]], dtype=np.int8), np.full((1, 3), -128, dtype=np.int8),
            {"ip": [49152, -48768, 0], "l2": [0, 3 * 255 * 255, 3 * 128 * 128]})


def rounding_pair(kind):
    """D = 1025: row 0 = 1024 x (128 or -128) then 0, row 1 the same then 1; the query is row 1.  The scores 2^24 and
    2^24 + 1 both convert to 16777216.0, so the rows are ordered by id, against the integer order."""
    base = np.zeros((2, 1025), dtype=DTYPE[kind])
    base[:, :1024] = 128 if kind == "u8" else -128
    base[1, 1024] = 1
    return base, base[1:2].copy()


def assert_same(got, want, what):
    gi, gd = got
    wi, wd = want
    bad_i = int((gi != wi).sum())
    bad_d = int((bits(gd) != bits(wd)).sum())
    print("%s: %d of %d ids and %d of %d float bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert gi.shape == wi.shape and bad_i == 0 and bad_d == 0, what


def assert_same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": lims"
    assert_same(got[1:], want[1:], what)


# ---- CPU ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_restatement_hand_answers(kind):
    base, q, answers = hand_case(kind)
    for metric, want in answers.items():
        assert B.table(base, q, metric)[0].tolist() == [float(x) for x in want]
    ids, s = B.search(B.table(base, q, "ip"), 3, "ip")
    assert ids.tolist() == [[0, 2, 1]]
    if kind == "i8":
        assert bits(s)[0, 1] == 0 and s[0, 2] == -48768.0          # an integer 0 is +0.0; the negative score comes last
        assert B.search(B.table(base, q, "l2"), 3, "l2")[0].tolist() == [[0, 2, 1]]


def test_restatement_largest_score_is_exact():
    full = np.full((1, 2048), 255, dtype=np.uint8)
    s = B.table(full, full, "ip")[0, 0]
    assert s == 133171200.0 and int(s) == 2048 * 65025 and 133171200 < 2 ** 31
    low = np.full((1, 2048), -128, dtype=np.int8)
    assert B.table(low, low, "ip")[0, 0] == 2.0 ** 25
    assert B.table(low, np.full((1, 2048), 127, dtype=np.int8), "l2")[0, 0] == 133171200.0


@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_restatement_rounding_pair_is_ordered_by_id(kind):
    base, q = rounding_pair(kind)
    exact = q.astype(np.int64) @ base.astype(np.int64).T
    assert exact.tolist() == [[2 ** 24, 2 ** 24 + 1]]
    ids, s = B.search(B.table(base, q, "ip"), 2, "ip")
    assert ids.tolist() == [[0, 1]] and bits(s).tolist() == [[int(np.float32(16777216).view(np.uint32))] * 2]


@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_restatement_equals_the_widened_ones(kind):
    rng = np.random.default_rng(5)
    base, qs = rand(rng, kind, (400, 37)), rand(rng, kind, (3, 37))
    base[:3] = base[5:8]                                               # exact ties
    wide, wq = base.astype(np.float32), qs.astype(np.float32)
    ip, l2 = B.table(base, qs, "ip"), B.table(base, qs, "l2")
    assert np.array_equal(bits(ip), bits(XI.all_scores(wide, wq)))
    assert np.array_equal(bits(l2), bits(np.stack([X.distances(wide, q) for q in wq])))
    direct = ((base.astype(np.int64)[None] - qs.astype(np.int64)[:, None]) ** 2).sum(-1)
    assert np.array_equal(l2, direct.astype(np.float32))              # the identity table() uses is the plain sum
    for k in (1, 100, 400):
        assert_same(B.search(ip, k, "ip", id_offset=7), XI.search(wide, wq, k, id_offset=7), "ip top-%d" % k)
        assert_same(B.search(l2, k, "l2", id_offset=7), X.search(wide, wq, k, id_offset=7), "l2 top-%d" % k)
    cand = rng.integers(-2, 407, size=(3, 50)).astype(np.int32)
    cand[cand >= 0] = np.clip(cand[cand >= 0], 7, 406)
    assert_same(B.rerank(base, qs, cand, 9, "ip", id_offset=7), XI.rerank(wide, wq, cand, 9, id_offset=7), "ip re-rank")
    assert_same(B.rerank(base, qs, cand, 9, "l2", id_offset=7), X.rerank(wide, wq, cand, 9, id_offset=7), "l2 re-rank")
    assert_same_lists(B.range_search(ip, np.float32(ip.mean()), "ip"), XI.range_search(wide, wq, np.float32(ip.mean())), "ip range")


def test_argument_errors_come_before_any_device_call(lib):
    """What can be refused without reading the handle is refused first: `fake` is never dereferenced."""
    from deltapq_amd import api
    fake = ctypes.c_void_p(0x1000)
    q = np.zeros((2, 8), dtype=np.uint8)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    t0, t_nan0, t_nan1 = np.float32([0, 0]), np.float32([np.nan, 1]), np.float32([0.5, np.nan])   # kept alive for the calls
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    res = ctypes.c_void_p()
    cases = {
        ("search", ""): [(None, p(q), 2, 4, p(i), p(s)), (fake, None, 2, 4, p(i), p(s)), (fake, p(q), 2, 4, None, p(s)),
                         (fake, p(q), 2, 4, p(i), None), (fake, p(q), -1, 4, p(i), p(s)), (fake, p(q), 2, 0, p(i), p(s)),
                         (fake, p(q), 2, 16385, p(i), p(s))],
        ("search_filtered", ""): [(None, fake, p(q), 2, 4, p(i), p(s)), (fake, None, p(q), 2, 4, p(i), p(s)),
                                  (fake, fake, None, 2, 4, p(i), p(s)), (fake, fake, p(q), 2, 4, None, p(s)),
                                  (fake, fake, p(q), 2, 4, p(i), None), (fake, fake, p(q), -1, 4, p(i), p(s)),
                                  (fake, fake, p(q), 2, 0, p(i), p(s)), (fake, fake, p(q), 2, 16385, p(i), p(s))],
        ("range_search", ""): [(fake, None, p(q), 2, p(t0), None), (None, None, p(q), 2, p(t0), ctypes.byref(res)),
                               (fake, None, p(q), -1, p(t0), ctypes.byref(res)), (fake, None, None, 2, p(t0), ctypes.byref(res)),
                               (fake, None, p(q), 2, None, ctypes.byref(res)), (fake, None, p(q), 2, p(t_nan1), ctypes.byref(res)),
                               (fake, fake, p(q), 2, p(t_nan0), ctypes.byref(res))],
        ("rerank", ""): [(None, p(q), 2, p(c), 4, 4, p(i), p(s)), (fake, None, 2, p(c), 4, 4, p(i), p(s)),
                         (fake, p(q), 2, None, 4, 4, p(i), p(s)), (fake, p(q), 2, p(c), 4, 4, None, p(s)),
                         (fake, p(q), 2, p(c), 4, 4, p(i), None), (fake, p(q), -1, p(c), 4, 4, p(i), p(s))],
        ("rerank", "_device"): [(None, fake, 2, fake, 4, 4, fake, fake, None), (fake, None, 2, fake, 4, 4, fake, fake, None),
                                (fake, fake, 2, None, 4, 4, fake, fake, None), (fake, fake, 2, fake, 4, 4, None, fake, None),
                                (fake, fake, 2, fake, 4, 4, fake, None, None), (fake, fake, -1, fake, 4, 4, fake, fake, None)],
    }
    for kind, metric in COMBOS:
        for (shape, tail), calls in cases.items():
            name = fn_name(shape, tail, kind, metric)
            for args in calls:
                assert getattr(lib, name)(*args) == -1, (name, args)
                assert name.encode() in lib.dpq_last_error()
        name = fn_name("range_search", "", kind, metric)
        assert getattr(lib, name)(fake, None, p(q), 2, p(t_nan1), ctypes.byref(res)) == -1
        what = b"threshold of query 1 is NaN" if metric == "ip" else b"radius of query 1 is NaN"
        assert what in lib.dpq_last_error() and res.value is None
        if api.device_count() == 0:       # the handle is read only after a device has been seen
            assert getattr(lib, fn_name("search_filtered", "", kind, metric))(fake, fake, p(q), 2, 4, p(i), p(s)) == -4
            assert getattr(lib, name)(fake, None, p(q), 2, p(t0), ctypes.byref(res)) == -4


def test_flat_open_i8_argument_errors_come_before_any_device_call(lib):
    from deltapq_amd import api
    v = np.zeros((4, 8), dtype=np.int8)

    def open_raw(ptr, n, D, device=0, id_offset=0, out=True):
        h = ctypes.c_void_p()
        return lib.dpq_flat_open_i8(ptr, n, D, device, id_offset, ctypes.byref(h) if out else None)
    pv = ctypes.c_void_p(v.ctypes.data)
    for args, kw in (((None, 4, 8), {}), ((pv, 4, 8), {"out": False}), ((pv, 0, 8), {}), ((pv, 4, 0), {}), ((pv, 4, 2049), {}),
                     ((pv, 4, 8), {"id_offset": -1}), ((pv, 4, 8), {"id_offset": 2 ** 31 - 4})):
        assert open_raw(*args, **kw) == -1, (args, kw)
        assert b"dpq_flat_open_i8" in lib.dpq_last_error()
    if api.device_count() == 0:                                            # ... and only then the device
        assert open_raw(pv, 4, 8) == -4
        with pytest.raises(api.DpqError) as e:
            api.FlatIndexI8(v)
        assert e.value.status == -4 and "no CPU fallback" in str(e.value)
    assert open_raw(pv, 4, 8, device=10 ** 6) == -4


def test_flat_index_i8_refuses_other_types_without_touching_the_library(monkeypatch):
    from deltapq_amd import _lib, api

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    for bad in (np.zeros((4, 8), dtype=np.uint8), np.zeros((4, 8), dtype=np.float32), [[1, 2], [3, 4]],
                np.zeros((8, 4), dtype=np.int8).T):                       # the last: int8, but not C-contiguous
        with pytest.raises(TypeError):
            api.FlatIndexI8(bad)
    with pytest.raises(TypeError):                                         # ... and FlatIndexU8 still refuses int8
        api.FlatIndexU8(np.zeros((4, 8), dtype=np.int8))


def test_cli_usage_text_is_unchanged(built):
    for task in ("groundtruth", "recall"):
        r = subprocess.run([EXE, "-task", task], capture_output=True, text=True)
        assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-metric l2|ip" in r.stdout and "[-ext fvecs|bvecs]" in r.stdout


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def open_index(gpu, kind, base, **kw):
    return (gpu.FlatIndexU8 if kind == "u8" else gpu.FlatIndexI8)(base, **kw)


def method(f, what, metric):
    return getattr(f, what + ("_ip" if metric == "ip" else ""))


def every_bound(metric):
    return np.float32(-np.inf if metric == "ip" else np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_gpu_hand_answers(gpu, kind):
    base, q, answers = hand_case(kind)
    metrics = [m for k, m in COMBOS if k == kind]
    with open_index(gpu, kind, base) as f:
        for metric in metrics:
            tab = B.table(base, q, metric)
            assert tab[0].tolist() == [float(x) for x in answers[metric]]
            want = B.search(tab, 3, metric)
            assert want[0].tolist() == [[0, 2, 1]]
            assert_same(method(f, "search", metric)(q, 3), want, "hand answers, search")
            cand = np.array([[2, 1, 0, -1]], dtype=np.int32)
            assert_same(method(f, "rerank", metric)(q, cand, 3), want, "hand answers, re-rank")
            got = method(f, "range_search", metric)(q, every_bound(metric))
            assert_same_lists(got, B.range_search(tab, every_bound(metric), metric), "hand answers, range")
            assert got[0].tolist() == [0, 3]
    pair, pq = rounding_pair(kind)
    full = np.full((3, 2048), 255 if kind == "u8" else -128, dtype=DTYPE[kind])
    for b, qq in ((pair, pq), (full, full[:1])):
        with open_index(gpu, kind, b) as f:
            for metric in metrics:
                tab = B.table(b, qq, metric)
                n = len(b)
                want = B.search(tab, n, metric)
                assert want[0][0].tolist() == list(range(n)) or metric == "l2"      # equal floats: by id
                assert_same(method(f, "search", metric)(qq, n), want, "rounding pair / largest score, search")
                cand = np.arange(n - 1, -1, -1, dtype=np.int32)[None, :]
                assert_same(method(f, "rerank", metric)(qq, cand, n), want, "rounding pair / largest score, re-rank")
                assert_same_lists(method(f, "range_search", metric)(qq, every_bound(metric)),
                                  B.range_search(tab, every_bound(metric), metric), "rounding pair / largest score, range")
                if metric == "ip":
                    assert want[1][0, 0] == (16777216.0 if b is pair else (133171200.0 if kind == "u8" else 2.0 ** 25))


# D, n, nq, top_k: 4099 is one stripe of 4096 rows plus three, 9000 three stripes (the threshold in force in the later
# ones), 65 queries a second query tile with 63 idle columns, D = 130 a second 128-byte chunk of the re-rank's staging
TILING = [(1, 255, 1, 1), (31, 257, 65, 100), (33, 4099, 1, 2048), (100, 9000, 65, 100), (130, 1, 1, 1), (130, 4099, 65, 1),
          (2048, 257, 1, 100), (100, 9000, 1, 2048)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,n,nq,top_k", TILING)
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_edges_of_the_tiling(gpu, kind, metric, D, n, nq, top_k):
    rng = np.random.default_rng(D * 100003 + n)
    base, qs = rand(rng, kind, (n, D)), rand(rng, kind, (nq, D))
    if D == 2048:                                  # the largest answers among ordinary rows
        base[5], qs[0] = (255, 255) if kind == "u8" else (-128, -128)
        if kind == "i8":
            base[7] = 127                          # against the query of -128s: the largest L2, 2048 * 255^2
    if n > 300:
        base[n - 2] = base[3]                      # an exact tie across the stripes
    tab = B.table(base, qs, metric)
    with open_index(gpu, kind, base, id_offset=11) as f:
        assert_same(method(f, "search", metric)(qs, top_k), B.search(tab, top_k, metric, id_offset=11),
                    "%s %s D %d n %d nq %d top-%d" % (kind, metric, D, n, nq, top_k))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_gpu_sign_handling_i8(gpu, metric):
    rng = np.random.default_rng(8)
    n, D = 3000, 8
    base = rng.choice(np.array([-128, -1, 0, 1, 127], dtype=np.int8), size=(n, D))
    base[:, 0] = 127
    base[10:20] = 0                                                        # zero rows: the score 0 against every query
    base[10:20, 0] = 127
    qs = rng.choice(np.array([-128, -1, 0, 1, 127], dtype=np.int8), size=(4, D))
    qs[0, 0] = 0                                                           # the zero rows score 0 against query 0
    qs[1] = 1
    qs[1, 0] = -128                                                        # 7 * 127 < 128 * 127: nothing but negative scores
    qs[2] = 0                                                              # nothing but zeros
    tab = B.table(base, qs, metric)
    if metric == "ip":
        assert (tab[1] < 0).all() and (tab[2] == 0).all() and (tab[0] > 0).any() and (tab[0] < 0).any() and (tab[0] == 0).any()
        assert len(np.unique(tab[0])) < n                                  # exact ties
    with gpu.FlatIndexI8(base) as f:
        for k in (1, 100, n):
            assert_same(method(f, "search", metric)(qs, k), B.search(tab, k, metric), "signs, top-%d" % k)
        bound = np.float32([0.0, -1000.0, -0.0, 5.0]) if metric == "ip" else np.float32([1e9, 30000.0, 16130.0, 0.0])
        assert_same_lists(method(f, "range_search", metric)(qs, bound), B.range_search(tab, bound, metric), "signs, range")


@pytest.fixture(scope="module")
def shared(gpu):
    """One data set per kind with the restatement's tables of both metrics, shared by the tests below and left unchanged."""
    out = {}
    rng = np.random.default_rng(31)
    for kind in ("u8", "i8"):
        base, qs = rand(rng, kind, (3000, 24)), rand(rng, kind, (5, 24))
        base[1000:1200] = base[0:200]                                      # exact ties
        base[2000:2010] = 0
        out[kind] = {"base": base, "qs": qs, "ip": B.table(base, qs, "ip"), "l2": B.table(base, qs, "l2")}
    return out


def masks(n):
    third = np.arange(n) % 3 == 0
    block = np.zeros(n, dtype=bool)
    block[1000:1500] = True
    few = np.zeros(n, dtype=bool)
    few[[3, 700, 701, 1100, 2999] + list(range(2000, 2032))] = True      # 37 rows: fewer than top_k
    return {"every third row": third, "one block": block, "fewer rows than top_k": few, "empty": np.zeros(n, dtype=bool)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_same_bits_as_the_fp32_path(gpu, shared, kind, metric):
    d = shared[kind]
    base, qs = d["base"], d["qs"]
    rng = np.random.default_rng(2)
    cand = rng.integers(0, len(base), size=(len(qs), 300)).astype(np.int32)
    cand[:, 5] = -1
    mask = masks(len(base))["every third row"]
    bound = np.float32(np.median(d[metric]))
    with open_index(gpu, kind, base) as f, gpu.FlatIndex(base.astype(np.float32)) as w:
        wq = qs.astype(np.float32)
        assert_same(method(f, "search", metric)(qs, 100), method(w, "search", metric)(wq, 100), "search against fp32")
        assert_same(method(f, "rerank", metric)(qs, cand, 50), method(w, "rerank", metric)(wq, cand, 50), "re-rank against fp32")
        assert_same_lists(method(f, "range_search", metric)(qs, bound), method(w, "range_search", metric)(wq, bound),
                          "range against fp32")
        with gpu.FlatIdFilter.from_mask(f, mask) as ff, gpu.FlatIdFilter.from_mask(w, mask) as wf:
            assert ff.n_allowed == int(mask.sum())
            assert_same(method(f, "search_filtered", metric)(qs, 100, ff), method(w, "search_filtered", metric)(wq, 100, wf),
                        "filtered search against fp32")
            assert_same_lists(method(f, "range_search", metric)(qs, bound, ff), method(w, "range_search", metric)(wq, bound, wf),
                              "filtered range against fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_filters(gpu, shared, kind, metric):
    d = shared[kind]
    base, qs, tab = d["base"], d["qs"], d[metric]
    bound = np.float32(np.median(tab))
    with open_index(gpu, kind, base) as f:
        for what, mask in masks(len(base)).items():
            with gpu.FlatIdFilter.from_mask(f, mask) as ff:
                want = B.search(tab, 100, metric, allowed=mask)
                assert_same(method(f, "search_filtered", metric)(qs, 100, ff), want, "filtered search, " + what)
                lists = B.range_search(tab, bound, metric, allowed=mask)
                assert_same_lists(method(f, "range_search", metric)(qs, bound, ff), lists, "filtered range, " + what)
                if what == "fewer rows than top_k":
                    assert (want[0][:, 37:] == -1).all() and (want[1][:, 37:] == (-np.inf if metric == "ip" else np.inf)).all()
                    assert (want[0][:, :37] >= 0).all()
                if what == "empty":
                    assert (want[0] == -1).all() and lists[0].tolist() == [0] * (len(qs) + 1) and len(lists[1]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_range_thresholds(gpu, kind, metric):
    rng = np.random.default_rng(12)
    lo, hi = (0, 8) if kind == "u8" else (-4, 4)                           # D = 2, eight values: long tie groups
    base = rng.integers(lo, hi, size=(3000, 2)).astype(DTYPE[kind])
    qs = rng.integers(lo, hi, size=(4, 2)).astype(DTYPE[kind])
    base[100:110] = 0                                                      # the score 0 against every query
    qs[2] = (0, 3)
    qs[3] = (1, 2) if kind == "u8" else (1, -2)
    tab = B.table(base, qs, metric)
    tie = np.sort(tab[3])[1500]
    assert (tab[3] == tie).sum() > 1 and (tab[3] > tie).any() and (tab[3] < tie).any()
    assert (tab[2] == 0).any() or metric == "l2"
    bound = np.float32([-np.inf, np.inf, -0.0, tie])                       # ip: all, none, s > +0.0, the tie group stays out
    want = B.range_search(tab, bound, metric)                              # l2: none, all, none, the tie group stays out
    sizes = np.diff(want[0]).tolist()
    assert sizes[:2] == ([3000, 0] if metric == "ip" else [0, 3000])
    assert sizes[2] == (int((tab[2] > 0).sum()) if metric == "ip" else 0)
    assert sizes[3] == int((tab[3] > tie).sum() if metric == "ip" else (tab[3] < tie).sum())
    with open_index(gpu, kind, base) as f:
        assert_same_lists(method(f, "range_search", metric)(qs, bound), want, "range thresholds")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand,top_k", [(1, 1), (100, 7), (16384, 1000)])
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_rerank(gpu, lib, kind, metric, n_cand, top_k):
    import torch
    rng = np.random.default_rng(n_cand)
    n, nq, off, D = 5000, 3, 300, 130
    base, qs = rand(rng, kind, (n, D)), rand(rng, kind, (nq, D))
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)
    if n_cand > 1:
        cand[:, 1] = cand[:, 0]                                            # a row named twice counts once
        cand[:, 3::7] = -1                                                 # negative candidates are padding
        cand[1, :] = -1                                                    # nothing but padding
    tq = torch.from_numpy(qs).cuda()
    with open_index(gpu, kind, base, id_offset=off) as f:
        want = B.rerank(base, qs, cand, top_k, metric, id_offset=off)
        assert_same(method(f, "rerank", metric)(qs, cand, top_k), want, "re-rank n_cand %d" % n_cand)
        on_device = getattr(f, "rerank_ip_torch" if metric == "ip" else "rerank_torch")
        ti, td = on_device(tq, torch.from_numpy(cand).cuda(), top_k)
        assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "re-rank on device tensors")
        bad = cand.copy()
        bad[0, 0] = off + n                                                # names no row: the host form, the device form's flag
        with pytest.raises(gpu.DpqError) as e:
            method(f, "rerank", metric)(qs, bad, top_k)
        assert e.value.status == -1 and "names no row" in str(e.value)
        with pytest.raises(gpu.DpqError) as e:
            on_device(tq, torch.from_numpy(bad).cuda(), top_k)
        assert e.value.status == -1 and "names no row" in str(e.value)
        if n_cand != 100:
            return
        # the n_cand rules, with a real handle: they are checked after the handle's kind
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        i, s = np.empty((nq, 8), dtype=np.int32), np.empty((nq, 8), dtype=np.float32)
        name = fn_name("rerank", "", kind, metric)
        for nc, k in ((100, 0), (100, 101), (16385, 7)):
            assert getattr(lib, name)(f._h, p(qs), nq, p(cand), nc, k, p(i), p(s)) == -1
            assert b"1 <= top_k <= n_cand <= 16384" in lib.dpq_last_error()
        # an id map with an even n_map: candidates are positions, n_map itself means the last one
        id_map = rng.permutation(n).astype(np.uint32)
        f.set_id_map(id_map)
        pos = rng.integers(0, n + 1, size=(nq, n_cand)).astype(np.int32)
        pos[:, 0] = n
        pos[:, 2] = -1
        want = B.rerank(base, qs, pos, top_k, metric, id_offset=off, id_map=id_map)
        assert_same(method(f, "rerank", metric)(qs, pos, top_k), want, "re-rank through an id map")
        pos[0, 0] = n + 1
        with pytest.raises(gpu.DpqError) as e:
            method(f, "rerank", metric)(qs, pos, top_k)
        assert e.value.status == -1


@pytest.mark.gpu
@pytest.mark.parametrize("kind,metric", COMBOS)
def test_gpu_parts_merge_to_the_whole(gpu, shared, kind, metric):
    d = shared[kind]
    base, qs, tab = d["base"], d["qs"], d[metric]
    cut, k = 1100, 100
    with open_index(gpu, kind, base[:cut]) as a, open_index(gpu, kind, base[cut:], id_offset=cut) as b:
        parts = [method(h, "search", metric)(qs, k) for h in (a, b)]
    merge = gpu.merge_topk_ip_host if metric == "ip" else gpu.merge_topk_host
    got = merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
    assert_same(got, B.search(tab, k, metric), "two parts merged")
    with open_index(gpu, kind, base) as f:
        assert_same(got, method(f, "search", metric)(qs, k), "two parts against one handle")


@pytest.mark.gpu
def test_gpu_handle_kinds(gpu, lib, shared):
    n, D = 70, 8
    q = np.zeros((2, D), dtype=np.uint8)                                   # 16 bytes: enough for every query type's read
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    t0 = np.float32([0, 0])
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    fake = ctypes.c_void_p(0x1000)                                         # the device forms' pointers: never read
    handles = {"f32": gpu.FlatIndex(np.zeros((n, D), dtype=np.float32)), "half": gpu.FlatIndexHalf(np.zeros((n, D), dtype=np.float32), "f16"),
               "u8": gpu.FlatIndexU8(np.zeros((n, D), dtype=np.uint8)), "i8": gpu.FlatIndexI8(np.zeros((n, D), dtype=np.int8))}
    try:
        for kind, metric in COMBOS:
            for held, h in handles.items():
                if held == kind:
                    continue
                right_kind = "f32" if held == "half" else held
                with gpu.FlatIdFilter.from_mask(h, np.ones(n, dtype=bool)) as ff:
                    for shape, tail in SHAPES:
                        name, right = fn_name(shape, tail, kind, metric), fn_name(shape, tail, right_kind, metric)
                        res = ctypes.c_void_p()
                        args = {"search": (h._h, p(q), 2, 4, p(i), p(s)), "search_filtered": (h._h, ff._h, p(q), 2, 4, p(i), p(s)),
                                "range_search": (h._h, None, p(q), 2, p(t0), ctypes.byref(res)),
                                "rerank": (h._h, p(q), 2, p(c), 4, 4, p(i), p(s)) if not tail else
                                          (h._h, fake, 2, fake, 4, 4, fake, fake, None)}[shape]
                        assert getattr(lib, name)(*args) == -1, (name, held)
                        msg = lib.dpq_last_error()
                        assert msg.startswith(name.encode() + b":") and msg.endswith(b"call " + right.encode()), msg
                        assert res.value is None
        # ... and the fp32-query inner product on a u8 handle now names the byte call
        assert lib.dpq_flat_search_ip(handles["u8"]._h, p(q.view(np.float32)), 1, 4, p(i), p(s)) == -1
        assert lib.dpq_last_error().endswith(b"call dpq_flat_search_ip_u8")
    finally:
        for h in handles.values():
            h.close()
    # the L2 calls of a u8 handle before and after an inner-product call has made the row sums: the same answers
    d = shared["u8"]
    base, qs = d["base"], d["qs"]
    mask = masks(len(base))["every third row"]
    with gpu.FlatIndexU8(base) as f, gpu.FlatIdFilter.from_mask(f, mask) as ff:
        def l2_answers():
            return f.search(qs, 100), f.search_filtered(qs, 100, ff), f.range_search(qs, 60000.0)[1:], \
                f.rerank(qs, np.tile(np.arange(200, dtype=np.int32), (len(qs), 1)), 20)
        before = l2_answers()
        assert_same(f.search_ip(qs, 100), B.search(d["ip"], 100, "ip"), "u8 inner product between the L2 calls")
        after = l2_answers()
        for x, y in zip(before, after):
            assert_same(y, x, "u8 L2 after the row sums exist")
        assert_same(before[0], B.search(d["l2"], 100, "l2"), "u8 L2 against the restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_gpu_cli_groundtruth_ip_over_bvecs(gpu, tmp_path, filtered):
    from deltapq_amd import synth
    rng = np.random.default_rng(17)
    d, n, nq, k = str(tmp_path), 3000, 5, 10
    base, qs = rand(rng, "u8", (n, 24)), rand(rng, "u8", (nq, 24))
    synth.write_bvecs(os.path.join(d, "base.bvecs"), base.astype(np.float32))
    synth.write_bvecs(os.path.join(d, "query.bvecs"), qs.astype(np.float32))
    extra = []
    mask = np.arange(n) % 3 == 0
    if filtered:
        gpu.write_bitmap(os.path.join(d, "allow.bin"), *gpu.FlatIdFilter.pack_mask(mask))
        extra = ["-filter", os.path.join(d, "allow.bin")]
    r = subprocess.run([EXE, "-dataset", d, "-task", "groundtruth", "-ext", "bvecs", "-topk", str(k), "-query_size", str(nq),
                        "-metric", "ip"] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    gt_path = os.path.join(d, "groundtruth", "N%dTop%d.ip%s.txt" % (n, k, ".filtered" if filtered else ""))
    assert gt_path in r.stdout
    with gpu.FlatIndex(base.astype(np.float32)) as w:
        if filtered:
            with gpu.FlatIdFilter.from_mask(w, mask) as wf:
                want = w.search_filtered_ip(qs.astype(np.float32), k, wf)
        else:
            want = w.search_ip(qs.astype(np.float32), k)
    assert_same(want, B.search(B.table(base, qs, "ip"), k, "ip", allowed=mask if filtered else None), "fp32 path against the restatement")
    gpu.write_groundtruth(os.path.join(d, "want.txt"), *want)
    assert open(gt_path, "rb").read() == open(os.path.join(d, "want.txt"), "rb").read()


@pytest.mark.gpu
def test_gpu_cli_chain_recall_ip_rerank_over_bvecs(gpu, tmp_path):
    """`-task recall -metric ip -rerank R -ext bvecs` re-ranks from a byte handle: the line it prints is the recall of
    FlatIndexU8.rerank_ip through the id map, which is FlatIndex's over the widened rows."""
    import re
    from deltapq_amd import synth
    d, n, nq, k, R = str(tmp_path), 4000, 12, 10, 100
    wide = synth.make_clustered_vectors(n, 128, seed=82, n_clusters=120, centre_seed=80)      # integers in 0 .. 218
    wq = synth.make_clustered_vectors(nq, 128, seed=83, n_clusters=120, centre_seed=80)
    base, qs = wide.astype(np.uint8), wq.astype(np.uint8)
    assert np.array_equal(base.astype(np.float32), wide) and np.array_equal(qs.astype(np.float32), wq)
    for name, v in (("learn", wide), ("base", wide), ("query", wq)):
        synth.write_bvecs(os.path.join(d, name + ".bvecs"), v)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256", "-ext", "bvecs"]
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq), "-metric", "ip"],
                 ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-rerank", str(R), "-metric", "ip"]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr   # a failed step ends the chain
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    _, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n), n)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        pos = idx.query_batch_ip(wq, R)[0]
    with gpu.FlatIndexU8(base) as f, gpu.FlatIndex(wide) as w:
        truth = f.search_ip(qs, k)
        assert_same(gpu.read_groundtruth(os.path.join(d, "groundtruth", "N%dTop%d.ip.txt" % (n, k))), truth, "ground-truth file")
        f.set_id_map(vec_id)
        w.set_id_map(vec_id)
        reranked = f.rerank_ip(qs, pos, k)
        assert_same(reranked, w.rerank_ip(wq, pos, k), "re-rank of the PQ answer against the fp32 handle")
        assert_same(reranked, B.rerank(base, qs, pos, k, "ip", id_map=vec_id), "re-rank of the PQ answer")
    got = re.search(r"^reranked recall@%d = ([0-9.]+)$" % k, r.stdout, re.M)
    assert got, r.stdout
    assert got.group(1) == "%.6f" % gpu.recall(reranked[0], truth[0], k=k, R=k)
