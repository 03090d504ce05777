"""Exact inner-product search over raw vectors (dpq_flat_*_ip, dpq_merge_topk_ip_host; include/deltapq_amd.h).  The rules
are restated in _exact_ip_restatement.py; the GPU is held to them bit for bit on ids and on score bits -- the order
(score descending, id ascending) is total, so no tie slack is needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _exact_ip_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")

A0, A1 = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -12)
# the four known answers of the contract, as rows of one base with D = 3 (a zero dimension adds +0.0), and a zero row
KNOWN_BASE = np.array([[A0, A1, 0],                        # 0: against KNOWN_QS[0] 0x3f801001
                       [2.0 ** 100, 1, -2.0 ** 100],       # 1: against ones 0.0 (any other order: 1.0)
                       [2.0 ** 30, 1, -2.0 ** 30],         # 2: against ones 1.0 (an fp32 accumulator: 0.0)
                       [-2.0 ** -80, 0, 0],                # 3: against KNOWN_QS[2] -2^-160 -> -0.0 -> +0.0
                       [0, 0, 0]], dtype=np.float32)       # 4: genuinely zero
KNOWN_QS = np.array([[A0, A1, 0], [1, 1, 1], [2.0 ** -80, 0, 0]], dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_restatement_known_answers():
    assert bits(X.scores(KNOWN_BASE[0:1, :2], KNOWN_QS[0, :2]))[0] == 0x3F801001
    p = np.float32(A0 * A0) + np.float32(A1 * A1)                         # products rounded to fp32 first
    assert bits(np.float32(p))[0] == 0x3F801000
    ones = np.ones(3, dtype=np.float32)
    assert bits(X.scores(KNOWN_BASE[1:2], ones))[0] == 0                  # (2^100 + 1) - 2^100 = 0 in order
    for perm in ([0, 2, 1], [2, 0, 1]):                                    # the 1 after the cancellation: 1.0
        assert X.scores(KNOWN_BASE[1:2, perm], ones)[0] == 1.0
    assert X.scores(KNOWN_BASE[2:3], ones)[0] == 1.0                      # fp64 holds 2^30 + 1
    acc = np.float32(0)
    for x in KNOWN_BASE[2]:
        acc = np.float32(acc + x)                                          # an fp32 accumulator loses the 1
    assert acc == 0.0
    tiny = X.scores(KNOWN_BASE[3:5, :1], KNOWN_QS[2, :1])
    assert bits(tiny).tolist() == [0, 0]                                   # -2^-160 -> -0.0 -> +0.0, and the zero row
    ids, s = X.search(KNOWN_BASE, KNOWN_QS[2:3], 5)
    assert ids.tolist() == [[1, 2, 0, 3, 4]] and bits(s[0, 3:]).tolist() == [0, 0]   # the two zeros tie: by id
    acc = np.float64(0)                                                    # a scalar loop agrees with the vectorised one
    for v, q in zip(KNOWN_BASE[0], KNOWN_QS[0]):
        acc = acc + np.float64(v) * np.float64(q)
    assert bits(np.float32(acc))[0] == 0x3F801001


def test_key_map_is_monotone_and_folds_the_zeros():
    s = np.array([np.inf, 3.5, 1.0, 1e-40, 0.0, -1e-40, -1.0, -np.inf], dtype=np.float32)
    w = X.word(bits(s)).astype(np.int64)
    assert (np.diff(w) > 0).all(), w
    assert w[-1] < 0xFFFFFFFF                                              # the padding key's word is above every score's
    assert X.word(bits(np.float32(-0.0))) == X.word(bits(np.float32(0.0))) == 0x7FFFFFFF
    assert np.array_equal(X.word(X.word(bits(s))), bits(s))               # its own inverse
    assert X.keys(np.float32([-0.0]), [7])[0] == X.keys(np.float32([0.0]), [7])[0]
    ids, sc = X.search(np.array([[2.0], [1.0], [-1.0], [3.0], [1.0]], dtype=np.float32), np.ones((1, 1), dtype=np.float32), 6,
                       id_offset=10)
    assert ids.tolist() == [[13, 10, 11, 14, 12, -1]] and sc.tolist() == [[3.0, 2.0, 1.0, 1.0, -1.0, -np.inf]]


def test_merge_topk_ip_host_on_hand_built_lists(lib):
    from deltapq_amd import api
    inf = np.inf
    ids = np.array([[[5, 9, 2, -1], [1, 3, -1, -1]],
                    [[4, 7, 2, 8], [-1, -1, -1, -1]],
                    [[6, -1, -1, -1], [3, 0, 2, -1]]], dtype=np.int32)
    sc = np.array([[[2.5, 0.0, -1.0, -inf], [-3.0, -3.0, -inf, -inf]],
                   [[2.5, 0.0, -1.0, -7.0], [-inf, -inf, -inf, -inf]],
                   [[-0.0, -inf, -inf, -inf], [-3.0, -3.0, -4.0, -inf]]], dtype=np.float32)
    oi, os_ = api.merge_topk_ip_host(ids, sc)
    # query 0: 2.5 twice (ids 4 < 5), then the zeros 0.0 / -0.0 / 0.0 by id (6, 7, 9): the first two of them
    assert oi[0].tolist() == [4, 5, 6, 7] and bits(os_[0]).tolist() == bits(np.float32([2.5, 2.5, 0.0, 0.0])).tolist()
    # query 1: four rows at -3 by id, the repeated row 3 kept twice
    assert oi[1].tolist() == [0, 1, 3, 3] and os_[1].tolist() == [-3.0] * 4
    assert np.array_equal(oi, X.merge(ids, sc)[0]) and np.array_equal(bits(os_), bits(X.merge(ids, sc)[1]))
    oi, os_ = api.merge_topk_ip_host(ids[:, 1:, :][1:2], sc[:, 1:, :][1:2])   # nothing but padding: -1 / -inf
    assert oi.tolist() == [[-1] * 4] and os_.tolist() == [[-inf] * 4]
    wide = api.merge_topk_ip_host(np.array([[[3, -1, -1]]], dtype=np.int32), np.float32([[[-2.0, 5.0, 5.0]]]))
    assert wide[0].tolist() == [[3, -1, -1]] and wide[1].tolist() == [[-2.0, -inf, -inf]]   # a padding row's score is ignored
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    o_i, o_s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    assert lib.dpq_merge_topk_ip_host(p(ids), p(sc), 3, 0, 4, p(o_i), p(o_s)) == 0       # nq == 0
    for args in ((None, p(sc), 3, 2, 4, p(o_i), p(o_s)), (p(ids), None, 3, 2, 4, p(o_i), p(o_s)),
                 (p(ids), p(sc), 3, 2, 4, None, p(o_s)), (p(ids), p(sc), 3, 2, 4, p(o_i), None),
                 (p(ids), p(sc), 0, 2, 4, p(o_i), p(o_s)), (p(ids), p(sc), 3, -1, 4, p(o_i), p(o_s)),
                 (p(ids), p(sc), 3, 2, 0, p(o_i), p(o_s))):
        assert lib.dpq_merge_topk_ip_host(*args) == -1
    assert b"dpq_merge_topk_ip_host" in lib.dpq_last_error()


def test_argument_errors_come_before_any_device_call(lib):
    """What can be refused without reading the handle is refused first: `fake` is never dereferenced."""
    from deltapq_amd import api
    fake = ctypes.c_void_p(0x1000)
    q = np.zeros((2, 8), dtype=np.float32)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    t0, t_nan0, t_nan1 = np.float32([0, 0]), np.float32([np.nan, 1]), np.float32([0.5, np.nan])   # kept alive for the calls
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    res = ctypes.c_void_p()
    for name, cases in (
        ("dpq_flat_search_ip", [(None, p(q), 2, 4, p(i), p(s)), (fake, None, 2, 4, p(i), p(s)), (fake, p(q), 2, 4, None, p(s)),
                                (fake, p(q), 2, 4, p(i), None), (fake, p(q), -1, 4, p(i), p(s)), (fake, p(q), 2, 0, p(i), p(s)),
                                (fake, p(q), 2, 16385, p(i), p(s))]),
        ("dpq_flat_search_filtered_ip", [(None, fake, p(q), 2, 4, p(i), p(s)), (fake, None, p(q), 2, 4, p(i), p(s)),
                                         (fake, fake, None, 2, 4, p(i), p(s)), (fake, fake, p(q), -1, 4, p(i), p(s)),
                                         (fake, fake, p(q), 2, 0, p(i), p(s)), (fake, fake, p(q), 2, 16385, p(i), p(s))]),
        ("dpq_flat_range_search_ip", [(fake, None, p(q), 2, p(t0), None),
                                      (None, None, p(q), 2, p(t0), ctypes.byref(res)),
                                      (fake, None, p(q), -1, p(t0), ctypes.byref(res)),
                                      (fake, None, None, 2, p(t0), ctypes.byref(res)),
                                      (fake, None, p(q), 2, None, ctypes.byref(res)),
                                      (fake, None, p(q), 2, p(t_nan1), ctypes.byref(res)),
                                      (fake, fake, p(q), 2, p(t_nan0), ctypes.byref(res))]),
        ("dpq_flat_rerank_ip", [(None, p(q), 2, p(c), 4, 4, p(i), p(s)), (fake, None, 2, p(c), 4, 4, p(i), p(s)),
                                (fake, p(q), 2, None, 4, 4, p(i), p(s)), (fake, p(q), 2, p(c), 4, 4, None, p(s)),
                                (fake, p(q), 2, p(c), 4, 4, p(i), None), (fake, p(q), -1, p(c), 4, 4, p(i), p(s))]),
        ("dpq_flat_rerank_ip_device", [(None, fake, 2, fake, 4, 4, fake, fake, None), (fake, None, 2, fake, 4, 4, fake, fake, None),
                                       (fake, fake, 2, None, 4, 4, fake, fake, None), (fake, fake, 2, fake, 4, 4, None, fake, None),
                                       (fake, fake, 2, fake, 4, 4, fake, None, None), (fake, fake, -1, fake, 4, 4, fake, fake, None)]),
    ):
        for args in cases:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert name.encode() in lib.dpq_last_error()
    assert lib.dpq_flat_range_search_ip(fake, None, p(q), 2, p(t_nan1), ctypes.byref(res)) == -1
    assert b"threshold of query 1 is NaN" in lib.dpq_last_error() and res.value is None
    if api.device_count() == 0:       # the handle is read only after a device has been seen
        assert lib.dpq_flat_search_filtered_ip(fake, fake, p(q), 2, 4, p(i), p(s)) == -4
        assert lib.dpq_flat_range_search_ip(fake, None, p(q), 2, p(t0), ctypes.byref(res)) == -4


def test_cli_usage_names_the_metric(built):
    for task in ("groundtruth", "recall"):
        r = subprocess.run([EXE, "-task", task], capture_output=True, text=True)
        assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-metric l2|ip" in r.stdout
    for extra in (["-metric", "cosine"], ["-metric", "ip", "-refine", "100"], ["-metric", "ip", "-gpus", "2"]):
        r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "recall", "-m", "8", "-k", "256", "-N", "100", "-query_size",
                            "1", "-topk", "1"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.startswith("usage: -metric l2|ip") and "-refine" in r.stdout and "-gpus" in r.stdout
    r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "query", "-m", "8", "-k", "256", "-metric", "ip"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout.startswith("usage: -metric l2|ip")


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
    print("%s: %d of %d ids and %d of %d score bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert gi.shape == wi.shape and bad_i == 0 and bad_d == 0, what


def assert_same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": lims"
    assert_same(got[1:], want[1:], what)


@pytest.mark.gpu
def test_gpu_known_answers(gpu):
    want = X.search(KNOWN_BASE, KNOWN_QS, 5)
    assert want[0][0].tolist() == [1, 2, 0, 4, 3] and bits(want[1][0])[2] == 0x3F801001
    assert want[0][1].tolist() == [0, 2, 1, 4, 3] and want[1][1][1] == 1.0 and bits(want[1][1][2:4]).tolist() == [0, 0]
    assert want[0][2].tolist() == [1, 2, 0, 3, 4] and bits(want[1][2][3:]).tolist() == [0, 0]
    with gpu.FlatIndex(KNOWN_BASE) as f:
        assert_same(f.search_ip(KNOWN_QS, 5), want, "known answers, search")
        cand = np.tile(np.array([4, 3, 2, 1, 0, -1], dtype=np.int32), (3, 1))
        assert_same(f.rerank_ip(KNOWN_QS, cand, 5), want, "known answers, re-rank")
        lims, ids, s = f.range_search_ip(KNOWN_QS, np.float32([-0.0, 0.0, -1.0]))
        assert_same_lists((lims, ids, s), X.range_search(KNOWN_BASE, KNOWN_QS, np.float32([-0.0, 0.0, -1.0])), "known answers, range")
        assert lims.tolist() == [0, 3, 5, 10]                              # -0.0 reads as +0.0: the zero row stays out


@pytest.mark.gpu
def test_gpu_handle_kinds(gpu, lib):
    base8 = np.zeros((70, 8), dtype=np.uint8)
    q = np.zeros((2, 8), dtype=np.float32)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    t0, t_nan0, t_nan1 = np.float32([0, 0]), np.float32([np.nan, 1]), np.float32([0.5, np.nan])   # kept alive for the calls
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    res = ctypes.c_void_p()
    with gpu.FlatIndexU8(base8) as f8, gpu.FlatIdFilter.from_mask(f8, np.ones(70, dtype=bool)) as ff:
        for rc in (lib.dpq_flat_search_ip(f8._h, p(q), 2, 4, p(i), p(s)),
                   lib.dpq_flat_search_filtered_ip(f8._h, ff._h, p(q), 2, 4, p(i), p(s)),
                   lib.dpq_flat_range_search_ip(f8._h, None, p(q), 2, p(t0), ctypes.byref(res)),
                   lib.dpq_flat_rerank_ip(f8._h, p(q), 2, p(c), 4, 4, p(i), p(s))):
            assert rc == -1
            msg = lib.dpq_last_error()
            assert b"byte vectors" in msg and b"no inner-product search" in msg and b"_ip" in msg


@pytest.mark.gpu
def test_gpu_search_integer_data_with_ties_and_negative_scores(gpu):
    rng = np.random.default_rng(21)
    base = rng.integers(-3, 4, size=(3000, 16)).astype(np.float32)
    base[1000:1500] = base[0:500]
    qs = rng.integers(-3, 4, size=(6, 16)).astype(np.float32)
    want = X.search(base, qs, 2500)
    tied = sum(int((np.diff(bits(row)) == 0).sum()) for row in want[1])
    print("exactly tied neighbours:", tied, "negative scores reported:", int((want[1] < 0).sum()))
    assert tied >= 1000 and (want[1] < 0).sum() >= 1000 and (want[1] == 0).any()
    with gpu.FlatIndex(base) as f:
        assert_same(f.search_ip(qs, 2500), want, "integer data")


@pytest.mark.gpu
@pytest.mark.parametrize("D,n,nq,top_k", [(1, 4099, 1, 1), (3, 4099, 65, 2048), (33, 4099, 3, 100), (100, 10007, 3, 10000)])
def test_gpu_search_shapes(gpu, D, n, nq, top_k):
    rng = np.random.default_rng(D * 7 + nq)
    base = rng.normal(size=(n, D)).astype(np.float32)
    qs = rng.normal(size=(nq, D)).astype(np.float32)
    with gpu.FlatIndex(base) as f:
        assert_same(f.search_ip(qs, top_k), X.search(base, qs, top_k), "D %d n %d nq %d top-%d" % (D, n, nq, top_k))
        ids, s = f.search_ip(qs[:0], top_k)      # nq == 0 is fine
        assert ids.shape == (0, top_k)
        with pytest.raises(gpu.DpqError) as e:
            f.search_ip(qs, n + 1 if n < 16384 else 16385)
        assert e.value.status == (-8 if n < 16384 else -1)


@pytest.mark.gpu
def test_gpu_search_every_stripe_lowers_the_threshold(gpu):
    """The base ordered by its score against the first query, worst first: every row beats that query's threshold so
    far; the second query is the first one negated, for which the same base is best first."""
    rng = np.random.default_rng(23)
    base = rng.normal(size=(30000, 8)).astype(np.float32)
    q = rng.normal(size=(1, 8)).astype(np.float32)
    qs = np.concatenate([q, -q])
    base = base[np.argsort(X.scores(base, qs[0]), kind="stable")]
    table = X.all_scores(base, qs)
    with gpu.FlatIndex(base) as f:
        assert_same(f.search_ip(qs, 100), X.search(base, qs, 100, table=table), "ordered base")
        assert_same(f.search_ip(qs, 3000), X.search(base, qs, 3000, table=table), "ordered base, top-3000")


@pytest.mark.gpu
def test_gpu_search_offsets_and_parts(gpu):
    rng = np.random.default_rng(24)
    base = rng.integers(-2, 3, size=(6001, 12)).astype(np.float32)    # many ties across the cut
    qs = rng.integers(-2, 3, size=(9, 12)).astype(np.float32)
    k, cut = 300, 2500
    with gpu.FlatIndex(base, id_offset=1000) as f:
        whole = f.search_ip(qs, k)
    assert_same(whole, X.search(base, qs, k, id_offset=1000), "id_offset")
    with gpu.FlatIndex(base[:cut], id_offset=1000) as a, gpu.FlatIndex(base[cut:], id_offset=1000 + cut) as b:
        ia, sa = a.search_ip(qs, k)
        ib, sb = b.search_ip(qs, k)
    assert_same(gpu.merge_topk_ip_host(np.stack([ia, ib]), np.stack([sa, sb])), whole, "two parts merged")


@pytest.fixture(scope="module")
def integer_case():
    rng = np.random.default_rng(25)
    base = rng.integers(-3, 4, size=(4500, 8)).astype(np.float32)
    qs = rng.integers(-3, 4, size=(6, 8)).astype(np.float32)
    masks = {"all": np.ones(4500, dtype=bool), "tenth": rng.random(4500) < 0.1, "one": np.arange(4500) == 4321,
             "none": np.zeros(4500, dtype=bool)}
    return base, qs, masks, X.all_scores(base, qs)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "tenth", "one", "none"])
def test_gpu_search_filtered(gpu, integer_case, which):
    base, qs, masks, table = integer_case
    mask, k = masks[which], 200
    want = X.search(base, qs, k, allowed=mask, table=table)
    with gpu.FlatIndex(base) as f, gpu.FlatIdFilter.from_mask(f, mask) as ff:
        assert ff.n_allowed == int(mask.sum())
        got = f.search_filtered_ip(qs, k, ff)
        assert_same(got, want, "filter '%s'" % which)
        if which == "all":
            assert_same(got, f.search_ip(qs, k), "a full filter and no filter")
        if which == "none":
            assert (got[0] == -1).all() and np.isneginf(got[1]).all()
        if which == "one":
            assert (got[0][:, 0] == 4321).all() and (got[0][:, 1:] == -1).all() and np.isneginf(got[1][:, 1:]).all()


@pytest.mark.gpu
def test_gpu_range_search(gpu, integer_case):
    base, qs, masks, table = integer_case
    inf = np.float32(np.inf)
    attained = np.float32([np.sort(table[q])[-1 - 40 * q] for q in range(len(qs))])     # scores some rows have exactly
    assert all((table[q] == attained[q]).any() for q in range(len(qs)))
    mixed = np.float32([attained[0], -inf, inf, 0.0, -0.0, table[5].min()])
    with gpu.FlatIndex(base) as f, gpu.FlatIdFilter.from_mask(f, masks["tenth"]) as ff:
        for thr, what in ((attained, "attained scores"), (-inf, "-inf"), (inf, "+inf"), (mixed, "mixed")):
            for mask, flt in ((None, None), (masks["tenth"], ff)):
                want = X.range_search(base, qs, thr, allowed=mask, table=table)
                got = f.range_search_ip(qs, thr, flt)
                assert_same_lists(got, want, "range, %s%s" % (what, ", filtered" if flt else ""))
                n_el = len(base) if mask is None else int(mask.sum())
                if what == "-inf":
                    assert np.diff(got[0]).tolist() == [n_el] * len(qs)
                if what == "+inf":
                    assert got[0].tolist() == [0] * (len(qs) + 1)
                if what == "attained scores":                                             # strictly above
                    for q in range(len(qs)):
                        assert (got[2][got[0][q]:got[0][q + 1]] > attained[q]).all()
        with pytest.raises(gpu.DpqError) as e:
            f.range_search_ip(qs, np.float32([0, 0, np.nan, 0, 0, 0]))
        assert e.value.status == -1


@pytest.mark.gpu
@pytest.mark.parametrize("n_cand,top_k,D", [(1, 1, 128), (100, 7, 100), (2048, 100, 128)])
def test_gpu_rerank_matches_the_restatement(gpu, n_cand, top_k, D):
    import torch
    rng = np.random.default_rng(n_cand + top_k)
    n, nq, off = 5000, 7, 300
    base = rng.integers(-4, 5, size=(n, D)).astype(np.float32) * np.float32(0.37)
    qs = rng.normal(size=(nq, D)).astype(np.float32)
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)     # with n_cand >= 100: duplicates
    cand[rng.random(size=cand.shape) < 0.2] = -1                               # padding
    if n_cand >= 100:
        cand[1, 5:] = -1                                                       # fewer valid candidates than top_k
        cand[2, :] = -1                                                        # none at all
        cand[3, :50] = cand[3, 50] = off + 17                                  # one row named 51 times ...
        base[17] = np.sign(qs[3]) * np.float32(4 * 0.37)                       # ... and the best row of its query
    with gpu.FlatIndex(base, id_offset=off) as f:
        want = X.rerank(base, qs, cand, top_k, id_offset=off)
        assert_same(f.rerank_ip(qs, cand, top_k), want, "rerank n_cand %d" % n_cand)
        ti, ts = f.rerank_ip_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(cand).cuda(), top_k)
        assert_same((ti.cpu().numpy(), ts.cpu().numpy()), want, "rerank on device tensors")
        if n_cand >= 100:
            assert (want[0][2] == -1).all() and np.isneginf(want[1][2]).all() and (want[0][1] == -1).sum() >= top_k - 5
            assert want[0][3][0] == off + 17 and (want[0][3] == off + 17).sum() == 1
        for bad_id in (off - 1, off + n):                                      # names no row: both variants refuse
            bad = cand.copy()
            bad[nq - 1, n_cand - 1] = bad_id
            with pytest.raises(gpu.DpqError) as e:
                f.rerank_ip(qs, bad, top_k)
            assert e.value.status == -1
            with pytest.raises(gpu.DpqError) as e:
                f.rerank_ip_torch(torch.from_numpy(qs).cuda(), torch.from_numpy(bad).cuda(), top_k)
            assert e.value.status == -1
        with pytest.raises(gpu.DpqError) as e:
            f.rerank_ip(qs, cand, n_cand + 1)
        assert e.value.status == -1


@pytest.mark.gpu
def test_gpu_rerank_with_a_map_and_the_even_n_rule(gpu):
    rng = np.random.default_rng(26)
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
        assert_same(f.rerank_ip(qs, cand, k), want, "rerank through a map")
        ids, _ = f.rerank_ip(qs, np.full((nq, 2), n_map, dtype=np.int32), 1)
        assert (ids[:, 0] == int(id_map[n_map - 1]) + 50).all()
        bad = cand.copy()
        bad[2, 3] = n_map + 1
        with pytest.raises(gpu.DpqError) as e:
            f.rerank_ip(qs, bad, k)
        assert e.value.status == -1


def _positions_to_ids(pos, vec_id):
    n = len(vec_id)
    p = np.where((pos == n) & (n % 2 == 0), n - 1, pos)
    return np.where(p >= 0, vec_id[np.clip(p, 0, n - 1)].astype(np.int64), -1).astype(np.int32)


N_E2E, NQ_E2E, K_E2E, R_E2E = 4000, 16, 20, 200


@pytest.fixture(scope="module")
def dataset(gpu, tmp_path_factory):
    """About 4000 clustered vectors with a codebook trained and an index built by the command line tool, once for the
    end-to-end tests: (directory, base, queries)."""
    from deltapq_amd import synth
    d = str(tmp_path_factory.mktemp("exact_ip"))
    base = synth.make_clustered_vectors(N_E2E, 128, seed=82, n_clusters=120, centre_seed=80)
    qs = synth.make_clustered_vectors(NQ_E2E, 128, seed=83, n_clusters=120, centre_seed=80)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), qs)
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(N_E2E), "-h", "1", "-diff", "8"]):
        r = subprocess.run([EXE, "-dataset", d, "-m", "8", "-k", "256"] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
    return d, base, qs


@pytest.fixture(scope="module")
def python_numbers(gpu, dataset):
    """The PQ inner-product answer, its exact re-rank through the id map, and the exact truth, through the Python face."""
    from deltapq_amd import synth
    d, base, qs = dataset
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    _, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, N_E2E))
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % N_E2E), N_E2E)
    with gpu.DeltaPQIndex.open_memory(payload, N_E2E, 8, 256, device=0) as idx, gpu.FlatIndex(base) as f:
        idx.set_codebook(cb)
        pos = idx.query_batch_ip(qs, R_E2E)[0]
        truth = f.search_ip(qs, K_E2E)
        f.set_id_map(vec_id)
        reranked = f.rerank_ip(qs, pos, K_E2E)
        everything = f.rerank_ip(qs, np.tile(np.arange(N_E2E, dtype=np.int32), (NQ_E2E, 1)), K_E2E)
    return {"vec_id": vec_id, "pos": pos, "truth": truth, "reranked": reranked, "everything": everything}


@pytest.mark.gpu
def test_gpu_end_to_end_rerank_does_not_lose_recall(gpu, dataset, python_numbers):
    _, base, qs = dataset
    pn = python_numbers
    found = _positions_to_ids(pn["pos"], pn["vec_id"])
    pq_recall = gpu.recall(found, pn["truth"][0], k=K_E2E, R=K_E2E)
    re_recall = gpu.recall(pn["reranked"][0], pn["truth"][0], k=K_E2E, R=K_E2E)
    print("recall@%d of the PQ inner-product answer %.4f, re-ranked from top-%d %.4f" % (K_E2E, pq_recall, R_E2E, re_recall))
    assert re_recall >= pq_recall
    assert pq_recall == X.recall(found, pn["truth"][0], K_E2E, K_E2E)
    assert_same(pn["truth"], X.search(base, qs, K_E2E), "exact truth")
    assert_same(pn["reranked"], X.rerank(base, qs, pn["pos"], K_E2E, id_map=pn["vec_id"]), "re-rank of the PQ answer")
    assert_same(pn["everything"], pn["truth"], "re-rank of all n rows")


@pytest.mark.gpu
def test_gpu_cli_chain_groundtruth_and_recall(gpu, dataset, python_numbers):
    d, base, qs = dataset
    pn = python_numbers
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256", "-metric", "ip"]
    env = dict(os.environ, DPQ_DEV="1", DPQ_GT_PART_ROWS="1500")      # three parts of the base
    r = subprocess.run(common + ["-task", "groundtruth", "-topk", str(K_E2E), "-query_size", str(NQ_E2E)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    gt_path = os.path.join(d, "groundtruth", "N%dTop%d.ip.txt" % (N_E2E, K_E2E))
    assert "in 3 part(s)" in r.stdout and gt_path in r.stdout
    assert_same(gpu.read_groundtruth(gt_path), pn["truth"], "ground-truth file")
    r = subprocess.run(common + ["-task", "recall", "-N", str(N_E2E), "-query_size", str(NQ_E2E), "-topk", str(K_E2E), "-rerank",
                                 str(R_E2E)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want_pq = gpu.recall(_positions_to_ids(pn["pos"], pn["vec_id"]), pn["truth"][0], k=K_E2E, R=K_E2E)
    want_re = gpu.recall(pn["reranked"][0], pn["truth"][0], k=K_E2E, R=K_E2E)
    got_pq = re.search(r"^recall@%d = ([0-9.]+)$" % K_E2E, r.stdout, re.M)
    got_re = re.search(r"^reranked recall@%d = ([0-9.]+)$" % K_E2E, r.stdout, re.M)
    assert got_pq and got_re, r.stdout
    print("CLI:", got_pq.group(0), "|", got_re.group(0), "| API: %.6f %.6f" % (want_pq, want_re))
    assert got_pq.group(1) == "%.6f" % want_pq and got_re.group(1) == "%.6f" % want_re
    # a filtered truth: the file name, and the rows of the Python answer
    mask = np.arange(N_E2E) % 3 == 0
    bitmap = os.path.join(d, "third.bitmap")
    gpu.write_bitmap(bitmap, *gpu.FlatIdFilter.pack_mask(mask))
    r = subprocess.run(common + ["-task", "groundtruth", "-topk", str(K_E2E), "-query_size", str(NQ_E2E), "-filter", bitmap],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with gpu.FlatIndex(base) as f, gpu.FlatIdFilter.from_mask(f, mask) as ff:
        want = f.search_filtered_ip(qs, K_E2E, ff)
    assert_same(gpu.read_groundtruth(os.path.join(d, "groundtruth", "N%dTop%d.ip.filtered.txt" % (N_E2E, K_E2E))), want,
                "filtered ground-truth file")
