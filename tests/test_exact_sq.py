"""Exact search over 8-bit and 4-bit scalar-quantised vectors (dpq_sq_train, dpq_sq_encode, dpq_sq_decode,
dpq_flat_open_sq, dpq_flat_open_quantised, dpq_flat_sq_get; include/deltapq_amd.h).  The quantiser's rules are restated in
_sq_restatement.py and met bit for bit; a quantised handle is held, bit for bit, to the fp32 handle over the decoded rows.
There is no tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _exact_ip_restatement as XI
import _exact_restatement as X
import _sq_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(pattern):
    return np.array([pattern], dtype=np.uint32).view(np.float32)


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_restatement_known_answers():
    lo, hi = f32(0x3DCCCCCD), f32(0x3F333333)                          # 0.1f, 0.7f
    assert lo[0] == np.float32(0.1) and hi[0] == np.float32(0.7)
    rows = np.stack([lo, hi])
    step8, step4 = S.train(rows, 8)[1], S.train(rows, 4)[1]
    assert bits_of(S.train(rows, 8)[0]).tolist() == [0x3DCCCCCD]
    assert bits_of(step8).tolist() == [0x3B1A33CD] and bits_of(step4).tolist() == [0x3D23D70A]
    v = np.float32([[0.4]])
    assert S.encode(v, lo, step8, 8).tolist() == [[128]] and S.encode(v, lo, step4, 4).tolist() == [[8]]
    assert bits_of(S.decode(np.uint8([[128]]), lo, step8, 8)).tolist() == [[0x3ECD6700]]
    assert bits_of(S.decode(np.uint8([[8]]), lo, step4, 4)).tolist() == [[0x3ED70A3D]]
    ties = np.float32([[0.5], [1.5], [2.5], [254.5], [255.5], [300], [-3]])
    assert S.encode(ties, np.float32([0]), np.float32([1]), 8)[:, 0].tolist() == [0, 2, 2, 254, 255, 255, 0]
    got = bits_of(S.decode(np.uint8([[111]]), f32(0x3EB0F069), f32(0x3B82A8A7), 8))[0, 0]
    fused = np.float32(float(f32(0x3EB0F069)[0]) + 111.0 * float(f32(0x3B82A8A7)[0]))    # one rounding: exact in fp64
    assert got == 0x3F49C676 and bits_of(fused)[()] == 0x3F49C675
    # -0.0 is stored as +0.0; a constant column has step +0.0, encodes to 0 and decodes to lo exactly
    lo0, st0 = S.train(np.float32([[-0.0, 2.5], [-0.0, 2.5]]), 8)
    assert bits_of(lo0).tolist() == [0, 0x40200000] and bits_of(st0).tolist() == [0, 0]
    assert S.encode(np.float32([[7, -7]]), lo0, st0, 8).tolist() == [[0, 0]]
    assert bits_of(S.decode(np.uint8([[200, 9]]), lo0, st0, 8)).tolist() == [[0, 0x40200000]]
    # storage: dimension 2j in the low nibble, the spare nibble of an odd D is 0 when written, ignored when read
    assert S.pack(np.uint8([[1, 2, 3]]), 4).tolist() == [[0x21, 0x03]]
    assert S.unpack(np.uint8([[0x21, 0xF3]]), 3, 4).tolist() == [[1, 2, 3]]


@pytest.mark.parametrize("bits", S.BITS)
def test_restatement_against_a_plain_double_loop(bits):
    rng = np.random.default_rng(bits)
    n, D, L = 40, 7, S.levels(bits)
    rows = (rng.normal(size=(n, D)) * 10.0 ** rng.integers(-2, 3, size=(1, D))).astype(np.float32)
    rows[:, 3] = np.float32(-1.25)                                     # a constant column
    rows[:, 4] = np.float32(-2) + rng.integers(0, 2 * L + 1, size=n).astype(np.float32) / 2   # ties under step 1
    rows[0, 4], rows[1, 4] = -2, -2 + L
    lo, step = S.train(rows, bits)
    assert step[4] == 1 and step[3] == 0
    for d in range(D):
        col = [float(x) for x in rows[:, d]]
        assert float(lo[d]) == min(col) and float(step[d]) == float(np.float32((max(col) - min(col)) / L))
    stored, wide = S.encode(rows, lo, step, bits), S.decode(S.encode(rows, lo, step, bits), lo, step, bits)
    halves = 0
    for r in range(n):
        for d in range(D):
            c = 0
            if float(step[d]) != 0.0:
                u = (float(rows[r, d]) - float(lo[d])) / float(step[d])
                halves += u - int(u) == 0.5
                c = int(min(max(round(u), 0), L))                      # round(): ties to even
            got = int(stored[r, d]) if bits == 8 else (int(stored[r, d // 2]) >> (4 * (d & 1))) & 15
            assert got == c, (r, d)
            prod = np.float32(float(c) * float(step[d]))               # the product of two floats is exact in fp64
            assert bits_of(wide[r, d])[()] == bits_of(np.float32(float(lo[d]) + float(prod)))[()], (r, d)
    assert halves >= 5
    if bits == 4:
        assert stored.shape == (n, 4) and (stored[:, 3] >> 4 == 0).all()


@pytest.mark.parametrize("bits", S.BITS)
def test_decode_matches_the_restatement(lib, bits):
    from deltapq_amd import api
    rng = np.random.default_rng(10 + bits)
    L = S.levels(bits)
    for D in (1, 2, 5, 16, 33):
        n = L + 1
        c = np.stack([np.roll(np.arange(n, dtype=np.uint8), d) for d in range(D)], axis=1)    # every code in every column
        lo = (rng.normal(size=D) * 10.0 ** rng.integers(-3, 4, size=D)).astype(np.float32)
        step = np.abs(rng.normal(size=D) * 10.0 ** rng.integers(-4, 2, size=D)).astype(np.float32)
        step[D // 2] = 0                                               # a constant column: every code reads lo
        stored = S.pack(c, bits)
        if bits == 4 and D % 2:
            stored[:, -1] |= 0xA0                                      # a spare nibble that must be ignored
        got, want = api.sq_decode(stored, lo, step, bits), S.decode(stored, lo, step, bits)
        bad = int((bits_of(got) != bits_of(want)).sum())
        print("bits %d D %d: %d of %d decoded values differ" % (bits, D, bad, want.size))
        assert got.shape == (n, D) and bad == 0
        assert (bits_of(got[:, D // 2]) == bits_of(lo[D // 2])).all()
    lo, step = np.concatenate([f32(0x3EB0F069), f32(0x3DCCCCCD)]), np.concatenate([f32(0x3B82A8A7), f32(0x3B1A33CD)])
    if bits == 8:                                                      # the unfused decode, through the library
        assert bits_of(api.sq_decode(np.uint8([[111, 128]]), lo, step, 8)).tolist() == [[0x3F49C676, 0x3ECD6700]]


def test_argument_errors_come_before_any_device_call(lib):
    """What can be refused without a device is refused first: `fake` is never dereferenced."""
    from deltapq_amd import api
    fake = ctypes.c_void_p(0x1000)
    D = 8
    lo, step = np.zeros(D, dtype=np.float32), np.ones(D, dtype=np.float32)
    bad_lo, nan_lo = lo.copy(), lo.copy()
    bad_lo[3], nan_lo[7] = np.inf, np.nan
    neg, nan_step, inf_step = step.copy(), step.copy(), step.copy()
    neg[0], nan_step[1], inf_step[2] = -1e-30, np.nan, np.inf
    h = ctypes.c_void_p(0x2000)
    out = ctypes.byref(h)
    # (function, arguments by name): data, n, D, bits, lo, step and, for the open calls, id_offset and out
    def call(name, data=fake, n=10, D=D, bits=8, lo=lo, step=step, off=0, out=out, res=fake):
        lo_p, step_p = (None if a is None else p(a) for a in (lo, step))
        fn = getattr(lib, name)
        if name == "dpq_sq_train":
            return fn(data, n, D, bits, 0, lo_p, step_p)
        if name == "dpq_sq_encode":
            return fn(data, n, D, bits, lo_p, step_p, 0, res)
        if name == "dpq_sq_decode":
            return fn(data, n, D, bits, lo_p, step_p, res)
        return fn(data, n, D, bits, lo_p, step_p, 0, off, out)
    every = ("dpq_sq_train", "dpq_sq_encode", "dpq_sq_decode", "dpq_flat_open_sq", "dpq_flat_open_quantised")
    opens = every[3:]
    takes_quantiser = every[1:]
    cases = [(every, dict(data=None), "NULL"), (every, dict(n=0), "n < 1"), (every, dict(n=-4), "n < 1"),
             (every, dict(D=0), "D outside"), (every, dict(D=2049), "D outside"),
             (every, dict(bits=0), "bits"), (every, dict(bits=6), "bits"), (every, dict(bits=16), "bits"),
             (every[:4], dict(lo=None), "NULL"), (every[:4], dict(step=None), "NULL"),
             (every[1:3], dict(res=None), "NULL"), (opens, dict(out=None), "NULL"),
             (opens, dict(off=-1), "id_offset"), (opens, dict(off=(1 << 31) - 10), "id_offset"),
             (takes_quantiser, dict(lo=bad_lo), "lo of dimension 3"), (takes_quantiser, dict(lo=nan_lo), "lo of dimension 7"),
             (takes_quantiser, dict(step=neg), "step of dimension 0"), (takes_quantiser, dict(step=nan_step), "step of dimension 1"),
             (takes_quantiser, dict(step=inf_step), "step of dimension 2"),
             (every[4:], dict(lo=None), "both"), (every[4:], dict(step=None), "both"),
             # the order: n before D before bits before id_offset before the quantiser's values
             (opens, dict(n=0, D=0, bits=5, off=-1, lo=bad_lo), "n < 1"), (opens, dict(D=0, bits=5, off=-1, lo=bad_lo), "D outside"),
             (opens, dict(bits=5, off=-1, lo=bad_lo), "bits"), (opens, dict(off=-1, lo=bad_lo), "id_offset")]
    for names, kw, what in cases:
        for name in names:
            assert call(name, **kw) == -1, (name, kw)
            msg = lib.dpq_last_error()
            assert name.encode() in msg and what.encode() in msg, (name, kw, msg)
    assert h.value is None                                             # *out is cleared wherever out is given
    assert lib.dpq_flat_sq_get(None, ctypes.byref(ctypes.c_int()), p(lo), p(step)) == -1
    if api.device_count() == 0:                                        # good arguments: the device is looked for next
        for name in ("dpq_sq_train", "dpq_sq_encode", "dpq_flat_open_sq", "dpq_flat_open_quantised"):
            assert call(name) == -4, name
        assert call("dpq_flat_open_quantised", lo=None, step=None, bits=4, off=(1 << 31) - 11) == -4


def test_python_face_refuses_what_it_cannot_take(lib):
    from deltapq_amd import api
    v, lo, step = np.zeros((3, 4), dtype=np.float32), np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.float32)
    c8, c4 = np.zeros((3, 4), dtype=np.uint8), np.zeros((3, 2), dtype=np.uint8)
    for call in (lambda: api.sq_train(v, bits=6), lambda: api.sq_encode(v, lo, step, bits=16), lambda: api.sq_decode(c8, lo, step, bits=2),
                 lambda: api.FlatIndexSQ(c8, lo, step, bits=5), lambda: api.FlatIndexSQ.from_float(v, bits=3),
                 lambda: api.sq_train(v[0]), lambda: api.sq_encode(v, lo[:3], step), lambda: api.sq_decode(c8, lo, step[:3]),
                 lambda: api.sq_decode(c8, lo, step, bits=4), lambda: api.FlatIndexSQ(c4, lo, step, bits=8),
                 lambda: api.FlatIndexSQ(c8[0], lo, step), lambda: api.FlatIndexSQ.from_float(v, lo=lo),
                 lambda: api.FlatIndexSQ.from_float(v, step=step), lambda: api.FlatIndexSQ.from_float(v, lo=lo[:2], step=step[:2])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: api.sq_train(v.astype(np.float64)), lambda: api.sq_encode(v.astype(np.float16), lo, step),
                 lambda: api.sq_encode(v, lo.astype(np.float64), step), lambda: api.sq_decode(c8.astype(np.int8), lo, step),
                 lambda: api.sq_decode(c8, lo, step.astype(np.float64)), lambda: api.FlatIndexSQ(v, lo, step),
                 lambda: api.FlatIndexSQ.from_float(c8), lambda: api.FlatIndexSQ.from_float(v, lo=lo, step=[1.0] * 4)):
        with pytest.raises(TypeError):
            call()
    assert issubclass(api.FlatIndexSQ, api.FlatIndex)


def test_cli_usage_names_the_quantised_stores(built):
    r = subprocess.run([EXE, "-task", "recall"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: deltapq" in r.stdout and "-store f16|bf16|sq8|sq4" in r.stdout
    for extra in (["-store", "sq6", "-rerank", "10"], ["-store", "sq8"], ["-store", "sq4"]):   # an unknown store; no re-rank
        r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "recall", "-m", "8", "-k", "256", "-N", "100", "-query_size",
                            "1", "-topk", "1"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.startswith("usage: -store f16|bf16|sq8|sq4"), r.stdout


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
    bad_d = int((bits_of(gd) != bits_of(wd)).sum())
    print("%s: %d of %d ids and %d of %d float bit patterns differ" % (what, bad_i, gi.size, bad_d, gd.size))
    assert gi.shape == wi.shape and bad_i == 0 and bad_d == 0, what


def assert_same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": lims"
    assert_same(got[1:], want[1:], what)


def assert_bits(got, want, what):
    bad = int((bits_of(got) != bits_of(want)).sum())
    print("%s: %d of %d float bit patterns differ" % (what, bad, np.asarray(want).size))
    assert np.asarray(got).shape == np.asarray(want).shape and bad == 0, what


def assert_codes(got, want, what):
    bad = int((got != want).sum())
    print("%s: %d of %d stored bytes differ" % (what, bad, want.size))
    assert got.dtype == np.uint8 and got.shape == want.shape and bad == 0, what


def make_rows(n, D, seed):
    """Random normals times a random power of ten per row, a tenth of the rows duplicated (ties go by id)."""
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=(n, D)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))).astype(np.float32)
    if n >= 10:
        dup = rng.choice(n, size=n // 10, replace=False)
        a[dup] = a[rng.integers(0, n, size=n // 10)]
    return a


def make_training_rows(n, D, bits, seed):
    """Columns of both signs and of different ranges; column 1 constant, column 2 on the half steps of a step of exactly
    1 (the ties), column 3 with -0.0 as its minimum; a tenth of the rows duplicated."""
    rng = np.random.default_rng(seed)
    L = S.levels(bits)
    a = (rng.normal(size=(n, D)) * 10.0 ** rng.integers(-2, 3, size=(1, D)) + rng.normal(size=(1, D))).astype(np.float32)
    if D > 1:
        a[:, 1] = np.float32(-1.25)
    if D > 2:
        a[:, 2] = np.float32(-2) + rng.integers(0, 2 * L + 1, size=n).astype(np.float32) / 2
        a[0, 2], a[-1, 2] = -2, -2 + L
    if D > 3:
        a[:, 3] = np.abs(a[:, 3])
        a[0, 3] = -0.0
    if n >= 10:
        dup = rng.choice(np.arange(1, n - 1), size=n // 10, replace=False)
        a[dup] = a[rng.integers(0, n, size=n // 10)]
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("bits", S.BITS)
@pytest.mark.parametrize("D", [1, 15, 16, 17, 31, 32, 33])
def test_gpu_train_and_encode_match_the_restatement(gpu, bits, D):
    for n in (1, 300):
        rows = make_training_rows(n, D, bits, 7 * D + bits + n)
        lo, step = gpu.sq_train(rows, bits)
        want_lo, want_step = S.train(rows, bits)
        assert_bits(lo, want_lo, "lo, bits %d D %d n %d" % (bits, D, n))
        assert_bits(step, want_step, "step, bits %d D %d n %d" % (bits, D, n))
        if n > 1 and D > 2:
            assert step[1] == 0 and step[2] == 1
            u = (rows[:, 2].astype(np.float64) + 2)
            assert (u - np.floor(u) == 0.5).sum() >= 20                # the ties are there
        if n > 1 and D > 3:
            assert bits_of(lo)[3] == 0                                 # -0.0 is stored as +0.0
        assert_codes(gpu.sq_encode(rows, lo, step, bits), S.encode(rows, lo, step, bits), "codes under the trained quantiser")
        # a caller's quantiser that covers a part of the values: the others saturate at both ends
        given_lo = (want_lo + (rows.max(axis=0) - want_lo) / 4).astype(np.float32)
        given_step = (want_step / 2).astype(np.float32) if n > 1 else np.full(D, 0.125, dtype=np.float32)
        got, want = gpu.sq_encode(rows, given_lo, given_step, bits), S.encode(rows, given_lo, given_step, bits)
        assert_codes(got, want, "codes under a caller's quantiser")
        if n > 1:
            c = S.unpack(want, D, bits)
            assert (c == 0).any() and (c == S.levels(bits)).any()


@pytest.mark.gpu
def test_gpu_train_encode_and_open_across_an_upload_slice(gpu):
    """Rows go up in slices of at most 128 MB: at D = 2048 a slice is 16384 rows, and this base has sixteen more."""
    n, D = 16400, 2048
    rng = np.random.default_rng(5)
    rows = rng.standard_normal(size=(n, D), dtype=np.float32)
    rows[16384:, 0] += 9                                               # the maximum of column 0 lies in the second slice
    rows[16383, 1] -= 9                                                # the minimum of column 1 at the end of the first
    lo, step = gpu.sq_train(rows, 8)
    want_lo, want_step = S.train(rows, 8)
    assert_bits(lo, want_lo, "lo across a slice")
    assert_bits(step, want_step, "step across a slice")
    got = gpu.sq_encode(rows, lo, step, 8)
    want = S.encode(rows[16370:], lo, step, 8)                         # the restatement of both sides of the boundary
    assert_codes(got[16370:], want, "codes across a slice")
    assert_codes(got[:30], S.encode(rows[:30], lo, step, 8), "codes of the first slice")
    qs = rows[16380:16390] + np.float32(0.01)
    cand = np.tile(np.arange(16370, 16400, dtype=np.int32), (len(qs), 1))
    with gpu.FlatIndexSQ.from_float(rows, 8) as a, gpu.FlatIndex(S.decode(want, lo, step, 8), id_offset=16370) as f:
        assert_same(a.rerank(qs, cand, 5), f.rerank(qs, cand, 5), "a quantised handle's rows on both sides of the slice")


@pytest.mark.gpu
@pytest.mark.parametrize("bits", S.BITS)
@pytest.mark.parametrize("n,D", [(300, 33), (65, 17), (1, 1), (700, 64)])
def test_gpu_open_quantised_is_the_composition_of_the_public_calls(gpu, bits, n, D):
    rows, qs = make_training_rows(n, D, bits, n + D + bits), make_rows(9, D, n + D)
    k = min(n, 20)
    for given in (False, True):
        if given:
            lo = np.full(D, -0.5, dtype=np.float32)
            step = np.full(D, 1 / 64, dtype=np.float32)
            a = gpu.FlatIndexSQ.from_float(rows, bits, lo=lo, step=step, id_offset=40)
        else:
            lo, step = gpu.sq_train(rows, bits)
            a = gpu.FlatIndexSQ.from_float(rows, bits, id_offset=40)
        stored = gpu.sq_encode(rows, lo, step, bits)
        dirty = stored.copy()
        if bits == 4 and D % 2:
            dirty[:, -1] |= 0xF0                                       # a spare nibble the open call must not store
        with a, gpu.FlatIndexSQ(dirty, lo, step, bits, id_offset=40) as b, gpu.FlatIndex(S.decode(stored, lo, step, bits), id_offset=40) as f:
            for h in (a, b):
                got_lo, got_step, got_bits = h.quantiser()
                assert got_bits == bits
                assert_bits(got_lo, lo, "the handle's lo")
                assert_bits(got_step, step, "the handle's step")
            for name in ("search", "search_ip"):
                want = getattr(f, name)(qs, k)
                assert_same(getattr(a, name)(qs, k), want, "%s, dpq_flat_open_quantised, bits %d, given %s" % (name, bits, given))
                assert_same(getattr(b, name)(qs, k), want, "%s, dpq_flat_open_sq, bits %d, given %s" % (name, bits, given))


SHAPES = [(1, 1, 1), (63, 5, 1), (65, 33, 65), (300, 100, 3), (9000, 32, 65), (9000, 128, 7)]


@pytest.fixture(scope="module")
def cases():
    """Per shape and width: the quantiser, the stored rows, the decoded rows and the queries, made once."""
    out = {}
    for n, D, nq in SHAPES:
        rows, qs = make_rows(n, D, n + D), make_rows(nq, D, n + D + 1)
        for bits in S.BITS:
            lo, step = S.train(rows, bits)
            stored = S.encode(rows, lo, step, bits)
            out[(n, D, nq, bits)] = (stored, lo, step, S.decode(stored, lo, step, bits), qs)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bits", S.BITS)
@pytest.mark.parametrize("n,D,nq", SHAPES)
def test_gpu_search_parity_with_the_fp32_handle(gpu, cases, n, D, nq, bits):
    stored, lo, step, wide, qs = cases[(n, D, nq, bits)]
    off = 1000 if (n, D) == (300, 100) else 0
    with gpu.FlatIndexSQ(stored, lo, step, bits, id_offset=off) as h, gpu.FlatIndex(wide, id_offset=off) as f:
        for top_k in sorted({1, min(10, n), min(100, n), min(n, 2048)}):
            assert_same(h.search(qs, top_k), f.search(qs, top_k), "L2 %d bits n %d D %d top-%d" % (bits, n, D, top_k))
            assert_same(h.search_ip(qs, top_k), f.search_ip(qs, top_k), "IP %d bits n %d D %d top-%d" % (bits, n, D, top_k))
        if (n, D) == (300, 100):                                       # and both against the restatements, once
            assert_same(h.search(qs, 10), X.search(wide, qs, 10, id_offset=off), "L2 restatement")
            assert_same(h.search_ip(qs, 10), XI.search(wide, qs, 10, id_offset=off), "IP restatement")
            assert_bits(gpu.sq_decode(stored, lo, step, bits), wide, "dpq_sq_decode")
        for call in (h.search, h.search_ip):
            with pytest.raises(gpu.DpqError) as e:
                call(qs, n + 1)
            assert e.value.status == -8
        assert h.search(qs[:0], 1)[0].shape == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", S.BITS)
@pytest.mark.parametrize("n,D,nq", [(9000, 32, 65), (65, 33, 65)])
def test_gpu_filtered_and_range_parity(gpu, cases, n, D, nq, bits):
    stored, lo, step, wide, qs = cases[(n, D, nq, bits)]
    inf = np.float32(np.inf)
    dist = np.stack([X.distances(wide, q) for q in qs])
    score = XI.all_scores(wide, qs)
    r10 = np.sort(dist, axis=1)[:, 9]                                  # each query's 10th-neighbour distance
    s10 = -np.sort(-score, axis=1)[:, 9]                               # and its 10th score
    masks = {"empty": np.zeros(n, dtype=bool), "one": np.arange(n) == n - 2, "every other": np.arange(n) % 2 == 1,
             "all": np.ones(n, dtype=bool)}
    with gpu.FlatIndexSQ(stored, lo, step, bits) as h, gpu.FlatIndex(wide) as f:
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
@pytest.mark.parametrize("bits", S.BITS)
@pytest.mark.parametrize("n_cand", [1, 100, 1000])
def test_gpu_rerank_parity_host_and_device(gpu, cases, bits, n_cand):
    import torch
    n, D, nq = 9000, 128, 7
    stored, lo, step, wide, qs = cases[(n, D, nq, bits)]
    rng = np.random.default_rng(n_cand)
    off, top_k = 300, min(n_cand, 40)
    cand = rng.integers(off, off + n, size=(nq, n_cand)).astype(np.int32)
    if n_cand >= 100:
        cand[rng.random(size=cand.shape) < 0.2] = -1                   # negative candidates are padding
        cand[1, 5:] = -1                                               # fewer valid candidates than top_k
        cand[2, :] = -1                                                # none at all
        cand[3, :50] = off + 17                                        # a row named fifty times
    tq = torch.from_numpy(qs).cuda()
    with gpu.FlatIndexSQ(stored, lo, step, bits, id_offset=off) as h, gpu.FlatIndex(wide, id_offset=off) as f:
        for hc, fc, ht, what in ((h.rerank, f.rerank, h.rerank_torch, "L2"), (h.rerank_ip, f.rerank_ip, h.rerank_ip_torch, "IP")):
            want = fc(qs, cand, top_k)
            assert_same(hc(qs, cand, top_k), want, "re-rank %s %d bits n_cand %d" % (what, bits, n_cand))
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
def test_gpu_handle_kinds(gpu, lib):
    q8 = np.zeros((2, 8), dtype=np.uint8)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    lo, step = np.zeros(8, dtype=np.float32), np.ones(8, dtype=np.float32)
    got_bits = ctypes.c_int(-1)
    for bits in S.BITS:
        h = gpu.FlatIndexSQ.from_float(np.zeros((70, 8), dtype=np.float32), bits)
        for name in ("dpq_flat_search_u8", "dpq_flat_search_i8", "dpq_flat_search_ip_u8"):
            assert getattr(lib, name)(h._h, p(q8), 2, 4, p(i), p(s)) == -1
            msg = lib.dpq_last_error()
            right = b"call dpq_flat_search_ip" if "_ip" in name else b"call dpq_flat_search"
            assert name.encode() in msg and b"scalar-quantised" in msg and msg.endswith(right), msg
        assert lib.dpq_flat_rerank_u8(h._h, p(q8), 2, p(c), 4, 4, p(i), p(s)) == -1
        msg = lib.dpq_last_error()
        assert b"dpq_flat_rerank_u8" in msg and b"scalar-quantised" in msg and msg.endswith(b"call dpq_flat_rerank")
        assert lib.dpq_flat_sq_get(h._h, ctypes.byref(got_bits), p(lo), p(step)) == 0 and got_bits.value == bits
        assert lib.dpq_flat_close(h._h) == 0                           # a quantised handle closes cleanly
        h._h = None
    with gpu.FlatIndex(np.zeros((70, 8), dtype=np.float32)) as f, gpu.FlatIndexHalf(np.zeros((70, 8), dtype=np.float32), "f16") as hf, \
            gpu.FlatIndexU8(np.zeros((70, 8), dtype=np.uint8)) as u:
        for other in (f, hf, u):
            assert lib.dpq_flat_sq_get(other._h, ctypes.byref(got_bits), p(lo), p(step)) == -1
            assert b"dpq_flat_sq_get" in lib.dpq_last_error()
        assert lib.dpq_flat_search_u8(f._h, p(q8), 2, 4, p(i), p(s)) == -1   # the other kinds answer as before
        assert b"the handle holds fp32 vectors (dpq_flat_open); call dpq_flat_search" in lib.dpq_last_error()


@pytest.mark.gpu
def test_gpu_cli_recall_with_a_quantised_store(gpu, tmp_path):
    """`-task recall -rerank R -store sq8`: the second re-rank line is the Python face's answer from a base quantised
    under the quantiser trained on it."""
    import re
    from deltapq_amd import synth
    n, nq, k, R, d = 3000, 16, 10, 100, str(tmp_path)
    base = synth.make_clustered_vectors(n, 64, seed=92, n_clusters=90, centre_seed=90) * np.float32(0.37)
    qs = synth.make_clustered_vectors(nq, 64, seed=93, n_clusters=90, centre_seed=90) * np.float32(0.37)
    for name, a in (("learn", base), ("base", base), ("query", qs)):
        synth.write_fvecs(os.path.join(d, name + ".fvecs"), a)
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    for args in (["-task", "learn"], ["-task", "encode"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "groundtruth", "-topk", str(k), "-query_size", str(nq)]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    _, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    vec_id = gpu.read_qnode_ids(os.path.join(d, "M8K256_Approx_TreeNodesDFS_N%d" % n), n)
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx, gpu.FlatIndex(base) as f:
        idx.set_codebook(cb)
        pos = idx.query_batch(qs, R)[0]
        truth = f.search(qs, k)[0]
    with gpu.FlatIndexSQ.from_float(base, 8) as h:
        h.set_id_map(vec_id)
        ids = h.rerank(qs, pos, k)[0]
    want = gpu.recall(ids, truth, k=k, R=k)
    r = subprocess.run(common + ["-task", "recall", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-rerank", str(R),
                                 "-store", "sq8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    fp32_line = re.search(r"^reranked recall@%d = ([0-9.]+)$" % k, r.stdout, re.M)
    sq_line = re.search(r"^reranked recall@%d \(sq8 store\) = ([0-9.]+)$" % k, r.stdout, re.M)
    assert fp32_line and sq_line, r.stdout
    print("CLI:", fp32_line.group(0), "|", sq_line.group(0), "| API: %.6f" % want)
    assert sq_line.group(1) == "%.6f" % want
