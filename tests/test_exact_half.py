"""Exact search over fp16 / bf16 vectors (dpq_flat_open_half, dpq_flat_open_narrowed, dpq_half_from_float,
dpq_half_to_float; include/deltapq_amd.h).  Widening a half to fp32 is exact, so there is no tolerance anywhere: a half
handle is held, bit for bit, to the fp32 handle over the widened rows, and the narrowing and widening to their
restatement in _half_restatement.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _exact_ip_restatement as XI
import _exact_restatement as X
import _half_restatement as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


def spread_values(n, seed, hi=5):
    """n fp32 values of both signs spread over 13 decades, 1e-8 .. 1e5: fp16's subnormal range and its overflow."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) * 10.0 ** rng.uniform(-8, hi, size=n)).astype(np.float32)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_restatement_agrees_with_numpy_and_torch():
    import torch
    v = np.concatenate([H.EDGES, H.EDGES_TO_INF, spread_values(100000, 1)])
    with np.errstate(over="ignore"):
        assert np.array_equal(H.narrow(v, "f16"), v.astype(np.float16).view(np.uint16))
    assert np.array_equal(H.narrow(v, "bf16"), torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    b = H.not_nan_patterns("f16")
    assert np.array_equal(bits(H.widen(b, "f16")), bits(b.view(np.float16).astype(np.float32)))


@pytest.mark.parametrize("fmt", H.FORMATS)
def test_half_from_float_matches_the_restatement(lib, fmt):
    from deltapq_amd import api
    f = lambda *x: api.half_from_float(np.float32(x), fmt).tolist()
    if fmt == "f16":
        assert f(2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20)) == [0x0001, 0x0000, 0x0001]
        assert f(65519.99, 65520.0, -65520.0) == [0x7BFF, 0x7C00, 0xFC00]
        assert f(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11) == [0x3C00, 0x3C02]
    else:
        assert f(1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20) == [0x3F80, 0x3F82, 0x3F81]
    assert f(0.0, -0.0) == [0x0000, 0x8000]
    v = np.concatenate([H.EDGES, H.EDGES_TO_INF, spread_values(100000, 2)])
    got, want = api.half_from_float(v, fmt), H.narrow(v, fmt)
    print("%s: %d of %d narrowed values differ" % (fmt, int((got != want).sum()), v.size))
    assert np.array_equal(got, want)
    assert api.half_from_float(v[:35].reshape(5, 7), fmt).shape == (5, 7)


@pytest.mark.parametrize("fmt", H.FORMATS)
def test_half_to_float_on_every_pattern_and_the_round_trip(lib, fmt):
    from deltapq_amd import api
    b = H.not_nan_patterns(fmt)
    assert len(b) == (65536 - 2 * 1023 if fmt == "f16" else 65536 - 2 * 127)
    wide = api.half_to_float(b, fmt)
    assert np.array_equal(bits(wide), bits(H.widen(b, fmt)))
    assert np.array_equal(api.half_from_float(wide, fmt), b)          # narrowing the widened value returns the pattern
    assert np.array_equal(H.narrow(H.widen(b, fmt), fmt), b)


def test_host_helper_argument_errors(lib):
    a, o = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.uint16)
    for name, src, dst in (("dpq_half_from_float", a, o), ("dpq_half_to_float", o, a)):
        fn = getattr(lib, name)
        assert fn(p(src), 4, 1, p(dst)) == 0 and fn(p(src), 4, 2, p(dst)) == 0 and fn(None, 0, 1, None) == 0
        for args in ((None, 4, 1, p(dst)), (p(src), 4, 1, None), (p(src), -1, 1, p(dst)), (p(src), 4, 0, p(dst)),
                     (p(src), 4, 3, p(dst))):
            assert fn(*args) == -1, (name, args)
            assert name.encode() in lib.dpq_last_error()


def test_argument_errors_come_before_any_device_call(lib):
    """What can be refused without a device is refused first: `fake` is never dereferenced."""
    from deltapq_amd import api
    fake = ctypes.c_void_p(0x1000)
    for name in ("dpq_flat_open_half", "dpq_flat_open_narrowed"):
        fn = getattr(lib, name)
        h = ctypes.c_void_p(0x2000)
        for args, what in (((None, 10, 8, 1, 0, 0, ctypes.byref(h)), "NULL"), ((fake, 10, 8, 1, 0, 0, None), "NULL"),
                           ((fake, 0, 8, 1, 0, 0, ctypes.byref(h)), "n < 1"), ((fake, -5, 8, 2, 0, 0, ctypes.byref(h)), "n < 1"),
                           ((fake, 10, 0, 1, 0, 0, ctypes.byref(h)), "D outside"), ((fake, 10, 2049, 2, 0, 0, ctypes.byref(h)), "D outside"),
                           ((fake, 10, 8, 1, 0, -1, ctypes.byref(h)), "id_offset"),
                           ((fake, 10, 8, 1, 0, (1 << 31) - 10, ctypes.byref(h)), "id_offset"),
                           ((fake, 10, 8, 0, 0, 0, ctypes.byref(h)), "format"), ((fake, 10, 8, 3, 0, 0, ctypes.byref(h)), "format")):
            assert fn(*args) == -1, (name, args)
            msg = lib.dpq_last_error()
            assert name.encode() in msg and what.encode() in msg, msg
        assert h.value is None                                         # *out is cleared wherever out is given
        if api.device_count() == 0:                                    # good arguments: the device is looked for next
            assert fn(fake, 10, 8, 1, 0, 0, ctypes.byref(h)) == -4
            assert fn(fake, 10, 8, 2, 0, (1 << 31) - 11, ctypes.byref(h)) == -4


def test_python_face_refuses_what_it_cannot_take(lib):
    from deltapq_amd import api
    with pytest.raises(ValueError):
        api.half_from_float(np.zeros(3, dtype=np.float32), "fp8")
    with pytest.raises(TypeError):
        api.half_to_float(np.zeros(3, dtype=np.float32), "f16")
    with pytest.raises(TypeError):
        api.FlatIndexHalf(np.zeros((3, 4), dtype=np.float16), "bf16")
    with pytest.raises(TypeError):
        api.FlatIndexHalf(np.zeros((3, 4), dtype=np.float64), "f16")
    assert issubclass(api.FlatIndexHalf, api.FlatIndex)


def test_cli_usage_names_the_store_switch(built):
    r = subprocess.run([EXE, "-task", "recall"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-store f16|bf16" in r.stdout
    for extra in (["-store", "fp8", "-rerank", "10"], ["-store", "f16"]):          # an unknown store; a store without a re-rank
        r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "recall", "-m", "8", "-k", "256", "-N", "100", "-query_size",
                            "1", "-topk", "1"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.startswith("usage: -store f16|bf16"), r.stdout


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
    print("%s: %d of %d ids and %d of %d float bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert gi.shape == wi.shape and bad_i == 0 and bad_d == 0, what


def assert_same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": lims"
    assert_same(got[1:], want[1:], what)


def make_rows(n, D, seed):
    """Random normals times a random power of ten per row, a tenth of the rows duplicated (ties go by id)."""
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=(n, D)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))).astype(np.float32)
    if n >= 10:
        dup = rng.choice(n, size=n // 10, replace=False)
        a[dup] = a[rng.integers(0, n, size=n // 10)]
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", H.FORMATS)
@pytest.mark.parametrize("D", [1, 3, 8, 9, 33])
def test_gpu_stored_bits_through_the_public_api(gpu, fmt, D):
    """Against the rows of the identity the score of row i under query d is the widened stored value of element (i, d):
    this pins the device narrowing, the padding and the widening of every element, for both ways of opening."""
    vals = np.concatenate([H.EDGES, spread_values(D * 40 - len(H.EDGES), 3 + D, hi=4)])    # every edge value, 40 rows
    if D == 1:                          # one term per score: a stored infinity reads back as itself
        vals = np.concatenate([vals, H.EDGES_TO_INF])
    base = vals.reshape(-1, D)
    n = len(base)
    stored = H.narrow(base, fmt)
    assert D == 1 or np.isfinite(H.widen(stored, fmt)).all()           # elsewhere inf * 0 would spoil a row's other scores
    want = H.widen(stored, fmt) + np.float32(0)                        # -0.0 reads +0.0
    eye = np.eye(D, dtype=np.float32)
    for how, src in (("dpq_flat_open_half", stored), ("dpq_flat_open_narrowed", base)):
        with gpu.FlatIndexHalf(src, fmt) as f:
            ids, s = f.search_ip(eye, n)
        got = np.empty((D, n), dtype=np.float32)
        for d in range(D):
            assert sorted(ids[d].tolist()) == list(range(n))
            got[d, ids[d]] = s[d]
        bad = int((bits(got.T) != bits(want)).sum())
        print("%s %s D %d: %d of %d stored values read back differently" % (how, fmt, D, bad, want.size))
        assert bad == 0


@pytest.mark.gpu
def test_gpu_known_answers(gpu):
    one = np.ones((1, 3), dtype=np.float32)
    with gpu.FlatIndexHalf(np.float32([[2.0 ** -24]]), "f16") as f:     # subnormals kept: flushed, this is 0.0
        assert f.search_ip(np.float32([[2.0 ** 24]]), 1)[1].tolist() == [[1.0]]
    with gpu.FlatIndexHalf(np.float32([[2.0 ** 15, 2.0 ** -10, -2.0 ** 15]]), "f16") as f:   # an fp32 accumulator gives 0
        assert f.search_ip(one, 1)[1].tolist() == [[2.0 ** -10]]
    with gpu.FlatIndexHalf(np.float32([[2.0 ** 100, 1, -2.0 ** 100]]), "bf16") as f:         # 0.0 only in order
        assert bits(f.search_ip(one, 1)[1]).tolist() == [[0]]
    row, q = np.float32([[1 + 2.0 ** -10, 2.0 ** -12]]), np.float32([[1, 0]])
    assert np.array_equal(H.widen(H.narrow(row, "f16"), "f16"), row)   # both values are halves
    want = X.search(row, q, 1)
    print("the L2 known answer: bits 0x%08x" % bits(want[1])[0, 0])
    with gpu.FlatIndexHalf(row, "f16") as f:
        assert_same(f.search(q, 1), want, "the L2 rule")
        assert_same(f.rerank(q, np.int32([[0]]), 1), want, "the L2 rule, re-rank")


SHAPES = [(1, 1, 1), (63, 5, 1), (65, 33, 65), (300, 100, 3), (9000, 32, 65), (9000, 128, 7)]


@pytest.fixture(scope="module")
def cases():
    """Per shape and format: the stored bits, the widened rows and the queries, made once."""
    out = {}
    for n, D, nq in SHAPES:
        rows, qs = make_rows(n, D, n + D), make_rows(nq, D, n + D + 1)
        for fmt in H.FORMATS:
            stored = H.narrow(rows, fmt)
            assert not (stored & 0x7FFF == (0x7C00 if fmt == "f16" else 0x7F80)).any()   # no infinities
            out[(n, D, nq, fmt)] = (stored, H.widen(stored, fmt), qs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", H.FORMATS)
@pytest.mark.parametrize("n,D,nq", SHAPES)
def test_gpu_search_parity_with_the_fp32_handle(gpu, cases, n, D, nq, fmt):
    stored, wide, qs = cases[(n, D, nq, fmt)]
    off = 1000 if (n, D) == (300, 100) else 0
    with gpu.FlatIndexHalf(stored, fmt, id_offset=off) as h, gpu.FlatIndex(wide, id_offset=off) as f:
        for top_k in sorted({1, min(10, n), min(n, 2048)}):
            assert_same(h.search(qs, top_k), f.search(qs, top_k), "L2 %s n %d D %d top-%d" % (fmt, n, D, top_k))
            assert_same(h.search_ip(qs, top_k), f.search_ip(qs, top_k), "IP %s n %d D %d top-%d" % (fmt, n, D, top_k))
        if (n, D) == (300, 100):                                       # and both against the restatements, once
            assert_same(h.search(qs, 10), X.search(wide, qs, 10, id_offset=off), "L2 restatement")
            assert_same(h.search_ip(qs, 10), XI.search(wide, qs, 10, id_offset=off), "IP restatement")
        for call in (h.search, h.search_ip):
            with pytest.raises(gpu.DpqError) as e:
                call(qs, n + 1)
            assert e.value.status == -8
        assert h.search(qs[:0], 1)[0].shape == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", H.FORMATS)
@pytest.mark.parametrize("n,D,nq", [(9000, 32, 65), (65, 33, 65)])
def test_gpu_filtered_and_range_parity(gpu, cases, n, D, nq, fmt):
    stored, wide, qs = cases[(n, D, nq, fmt)]
    inf = np.float32(np.inf)
    dist = np.stack([X.distances(wide, q) for q in qs])
    score = XI.all_scores(wide, qs)
    r10 = np.sort(dist, axis=1)[:, 9]                                  # each query's 10th-neighbour distance
    s10 = -np.sort(-score, axis=1)[:, 9]                               # and its 10th score
    masks = {"empty": np.zeros(n, dtype=bool), "one": np.arange(n) == n - 2, "every other": np.arange(n) % 2 == 1,
             "all": np.ones(n, dtype=bool)}
    with gpu.FlatIndexHalf(stored, fmt) as h, gpu.FlatIndex(wide) as f:
        for name, mask in masks.items():
            with gpu.FlatIdFilter.from_mask(h, mask) as hf, gpu.FlatIdFilter.from_mask(f, mask) as ff:
                assert hf.n_allowed == ff.n_allowed == int(mask.sum())
                for k in (1, 10):
                    assert_same(h.search_filtered(qs, k, hf), f.search_filtered(qs, k, ff), "filtered L2, %s" % name)
                    assert_same(h.search_filtered_ip(qs, k, hf), f.search_filtered_ip(qs, k, ff), "filtered IP, %s" % name)
                if name in ("every other", "one"):
                    assert_same_lists(h.range_search(qs, r10, hf), f.range_search(qs, r10, ff), "range L2, %s" % name)
                    assert_same_lists(h.range_search_ip(qs, s10, hf), f.range_search_ip(qs, s10, ff), "range IP, %s" % name)
                if name == "all":                                      # a filter made on another handle
                    for call in (lambda: h.search_filtered(qs, 1, ff), lambda: h.range_search_ip(qs, 0.0, ff),
                                 lambda: f.search_filtered_ip(qs, 1, hf)):
                        with pytest.raises(gpu.DpqError) as e:
                            call()
                        assert e.value.status == -1 and "another handle" in str(e.value)
        for r, what in ((r10, "10th distance"), (inf, "+inf"), (np.float32(0), "0")):
            got = h.range_search(qs, r)
            assert_same_lists(got, f.range_search(qs, r), "range L2, radius %s" % what)
            if what == "+inf":
                assert np.diff(got[0]).tolist() == [n] * nq
            if what == "0":
                assert got[0].tolist() == [0] * (nq + 1)
            if what == "10th distance":                                # strictly below: at most nine rows
                assert (np.diff(got[0]) <= 9).all() and np.diff(got[0]).max() >= 1
        for t, what in ((s10, "10th score"), (-inf, "-inf"), (inf, "+inf")):
            got = h.range_search_ip(qs, t)
            assert_same_lists(got, f.range_search_ip(qs, t), "range IP, threshold %s" % what)
            if what == "-inf":
                assert np.diff(got[0]).tolist() == [n] * nq
            if what == "+inf":
                assert got[0].tolist() == [0] * (nq + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", H.FORMATS)
@pytest.mark.parametrize("n_cand", [1, 100, 1000])
def test_gpu_rerank_parity_host_and_device(gpu, cases, fmt, n_cand):
    import torch
    n, D, nq = 9000, 128, 7
    stored, wide, qs = cases[(n, D, nq, fmt)]
    rng = np.random.default_rng(n_cand)
    off, top_k = 300, min(n_cand, 40)
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)
    if n_cand >= 100:
        cand[rng.random(size=cand.shape) < 0.2] = -1                   # negative candidates are padding
        cand[1, 5:] = -1                                               # fewer valid candidates than top_k
        cand[2, :] = -1                                                # none at all
        cand[3, :50] = off + 17                                        # a row named fifty times
    tq = torch.from_numpy(qs).cuda()
    with gpu.FlatIndexHalf(stored, fmt, id_offset=off) as h, gpu.FlatIndex(wide, id_offset=off) as f:
        for hc, fc, ht, what in ((h.rerank, f.rerank, h.rerank_torch, "L2"), (h.rerank_ip, f.rerank_ip, h.rerank_ip_torch, "IP")):
            want = fc(qs, cand, top_k)
            assert_same(hc(qs, cand, top_k), want, "re-rank %s %s n_cand %d" % (what, fmt, n_cand))
            ti, td = ht(tq, torch.from_numpy(cand).cuda(), top_k)
            assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "re-rank %s on device tensors" % what)
            if n_cand >= 100:
                assert (want[0][2] == -1).all() and (want[0][3] == off + 17).sum() <= 1
            for bad_id in (off - 1, off + n):                          # names no row: the host check, the flag word
                bad = cand.copy()
                bad[nq - 1, n_cand - 1] = bad_id
                with pytest.raises(gpu.DpqError) as e:
                    hc(qs, bad, top_k)
                assert e.value.status == -1
                with pytest.raises(gpu.DpqError) as e:
                    ht(tq, torch.from_numpy(bad).cuda(), top_k)
                assert e.value.status == -1 and "names no row" in str(e.value)
        assert_same(h.rerank(qs, cand, top_k), X.rerank(wide, qs, cand, top_k, id_offset=off), "re-rank, the restatement")
        # an id map with an even n_map: candidate n_map names the last position
        n_map = 2000
        id_map = rng.permutation(n)[:n_map].astype(np.uint32)
        pos = rng.integers(0, n_map - 1, size=(nq, n_cand)).astype(np.int32)
        pos[:, 0] = n_map
        h.set_id_map(id_map)
        f.set_id_map(id_map)
        assert_same(h.rerank(qs, pos, top_k), f.rerank(qs, pos, top_k), "re-rank L2 through a map")
        assert_same(h.rerank_ip(qs, pos, top_k), f.rerank_ip(qs, pos, top_k), "re-rank IP through a map")
        ids, _ = h.rerank_ip(qs, np.full((nq, 1), n_map, dtype=np.int32), 1)
        assert (ids[:, 0] == int(id_map[n_map - 1]) + off).all()
        pos[0, 0] = n_map + 1
        with pytest.raises(gpu.DpqError) as e:
            h.rerank(qs, pos, top_k)
        assert e.value.status == -1


@pytest.mark.gpu
def test_gpu_handle_kinds_and_the_format_argument(gpu, lib, cases):
    q8 = np.zeros((2, 8), dtype=np.uint8)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    h = gpu.FlatIndexHalf(np.zeros((70, 8), dtype=np.float32), "bf16")
    assert lib.dpq_flat_search_u8(h._h, p(q8), 2, 4, p(i), p(s)) == -1
    msg = lib.dpq_last_error()
    assert b"dpq_flat_search_u8" in msg and b"half-precision" in msg and msg.endswith(b"call dpq_flat_search")
    assert lib.dpq_flat_rerank_u8(h._h, p(q8), 2, p(c), 4, 4, p(i), p(s)) == -1
    msg = lib.dpq_last_error()
    assert b"dpq_flat_rerank_u8" in msg and b"half-precision" in msg and msg.endswith(b"call dpq_flat_rerank")
    assert lib.dpq_flat_close(h._h) == 0                               # a half handle closes cleanly
    h._h = None
    with gpu.FlatIndex(np.zeros((70, 8), dtype=np.float32)) as f:     # the other kinds answer as before
        assert lib.dpq_flat_search_u8(f._h, p(q8), 2, 4, p(i), p(s)) == -1
        assert b"the handle holds fp32 vectors (dpq_flat_open); call dpq_flat_search" in lib.dpq_last_error()
    # two formats over the same fp32 rows differ exactly where the restatement says they do
    rows, qs = make_rows(300, 16, 77), np.eye(16, dtype=np.float32)
    with gpu.FlatIndexHalf(rows, "f16") as a, gpu.FlatIndexHalf(rows, "bf16") as b:
        got, answers = [], {}
        for f, fmt in ((a, "f16"), (b, "bf16")):
            ids, sc = answers[fmt] = f.search_ip(qs, 300)
            t = np.empty((16, 300), dtype=np.float32)
            for d in range(16):
                t[d, ids[d]] = sc[d]
            assert np.array_equal(bits(t.T), bits(H.widen(H.narrow(rows, fmt), fmt) + np.float32(0)))
            got.append(t.T)
    # the other things the Python face takes: a float16 array, a CPU tensor of the format's dtype
    import torch
    with gpu.FlatIndexHalf(H.narrow(rows, "f16").view(np.float16), "f16") as a, \
            gpu.FlatIndexHalf(torch.from_numpy(rows).to(torch.bfloat16), "bf16") as b, \
            gpu.FlatIndexHalf(torch.from_numpy(rows).to(torch.float16), "f16") as c:
        assert_same(a.search_ip(qs, 300), answers["f16"], "a float16 array")
        assert_same(b.search_ip(qs, 300), answers["bf16"], "a bfloat16 tensor")
        assert_same(c.search_ip(qs, 300), answers["f16"], "a float16 tensor")
    differ = bits(got[0]) != bits(got[1])
    want = bits(H.widen(H.narrow(rows, "f16"), "f16") + np.float32(0)) != bits(H.widen(H.narrow(rows, "bf16"), "bf16") + np.float32(0))
    print("the two formats differ on %d of %d values" % (int(differ.sum()), differ.size))
    assert np.array_equal(differ, want) and differ.sum() > differ.size // 2


@pytest.mark.gpu
def test_gpu_cli_recall_with_a_half_store(gpu, tmp_path):
    """`-task recall -rerank R -store f16|bf16`: the second re-rank line is the Python face's answer from a narrowed base."""
    import re
    from deltapq_amd import synth
    n, nq, k, R, d = 3000, 16, 10, 100, str(tmp_path)
    base = synth.make_clustered_vectors(n, 64, seed=92, n_clusters=90, centre_seed=90) * np.float32(0.37)   # not exact in 16 bits
    qs = synth.make_clustered_vectors(nq, 64, seed=93, n_clusters=90, centre_seed=90) * np.float32(0.37)
    for name, a in (("learn", base), ("base", base), ("query", qs)):
        synth.write_fvecs(os.path.join(d, name + ".fvecs"), a)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq), "-metric", "ip"]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    _, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n), n)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx, gpu.FlatIndex(base) as f:
        idx.set_codebook(cb)
        pos = {"l2": idx.query_batch(qs, R)[0], "ip": idx.query_batch_ip(qs, R)[0]}
        truth = {"l2": f.search(qs, k)[0], "ip": f.search_ip(qs, k)[0]}
    for fmt, metric in (("f16", "l2"), ("bf16", "ip")):
        with gpu.FlatIndexHalf(base, fmt) as h:
            h.set_id_map(vec_id)
            ids = (h.rerank if metric == "l2" else h.rerank_ip)(qs, pos[metric], k)[0]
        want = gpu.recall(ids, truth[metric], k=k, R=k)
        r = subprocess.run(common + ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-rerank", str(R),
                                     "-store", fmt, "-metric", metric], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        fp32_line = re.search(r"^reranked recall@%d = ([0-9.]+)$" % k, r.stdout, re.M)
        half_line = re.search(r"^reranked recall@%d \(%s store\) = ([0-9.]+)$" % (k, fmt), r.stdout, re.M)
        assert fp32_line and half_line, r.stdout
        print("CLI:", fp32_line.group(0), "|", half_line.group(0), "| API: %.6f" % want)
        assert half_line.group(1) == "%.6f" % want
