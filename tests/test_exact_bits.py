"""Exact Hamming search over packed binary vectors (dpq_flat_open_bits, dpq_flat_*_bits): the numpy
restatement against the fp32 restatement on 0/1 rows, the argument checks and the Python face without a GPU, and on the
GPU ids and distance bits equal to the restatement at the padding, tile, stripe and tie edges, against the byte handle
over the unpacked rows, under filters, radii, re-ranking, binarising, the handle kinds and the command line."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _exact_bits_restatement as B
import _exact_restatement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def random_packed(n, D, seed, dup=0.1):
    """Random packed rows, spare bits 0, a tenth of them copies of other rows (ties go by id)."""
    rng = np.random.default_rng(seed)
    rows = B.pack_bits(rng.integers(0, 2, size=(n, D), dtype=np.uint8))
    if n > 1 and dup:
        k = max(1, int(n * dup))
        rows[rng.integers(0, n, size=k)] = rows[rng.integers(0, n, size=k)]
    return rows


def with_spare(packed, D, ones):
    """The same rows with the spare bits of the last byte all ones, or all zeros."""
    out = B.mask_spare(packed, D)
    if ones and D % 8:
        out[:, -1] |= np.uint8(0xFF & ~((1 << (D % 8)) - 1))
    return out


# ---- without a GPU --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [1, 9, 130])
def test_restatement_agrees_with_the_fp32_restatement_on_unpacked_rows(D):
    """Squared L2 of 0/1 vectors is their Hamming distance: ids and distance bits, top_k in (1, 100, n)."""
    n, nq = 150, 4
    base, queries = random_packed(n, D, seed=D), random_packed(nq, D, seed=100 + D, dup=0)
    # spare bits are ignored: fill them on one side
    base_s, queries_s = with_spare(base, D, True), with_spare(queries, D, False)
    b01, q01 = B.unpack_bits(base, D).astype(np.float32), B.unpack_bits(queries, D).astype(np.float32)
    for top_k in (1, 100, n):
        gi, gd = B.search(base_s, queries_s, D, top_k, id_offset=3)
        wi, wd = X.search(b01, q01, top_k, id_offset=3)
        assert np.array_equal(gi, wi) and np.array_equal(bits_of(gd), bits_of(wd)), (D, top_k)
    cand = np.random.default_rng(D).integers(-1, n, size=(nq, 40)).astype(np.int32)
    gi, gd = B.rerank(base_s, queries_s, D, cand, 10)
    wi, wd = X.rerank(b01, q01, cand, 10)
    assert np.array_equal(gi, wi) and np.array_equal(bits_of(gd), bits_of(wd))


def test_restatement_known_answers():
    base = np.uint8([[0b00000101, 0xFF], [0b00000101, 0x01], [0, 0]])          # D = 9: only bit 0 of the second byte counts
    q = np.uint8([[0b00000100, 0xFE]])
    assert B.all_distances(base, q, 9).tolist() == [[2.0, 2.0, 1.0]]
    i, d = B.search(base, q, 9, 4, id_offset=10)
    assert i.tolist() == [[12, 10, 11, -1]] and d[0, :3].tolist() == [1.0, 2.0, 2.0] and np.isinf(d[0, 3])
    lims, ids, ds = B.range_search(base, q, 9, 2.0)
    assert lims.tolist() == [0, 1] and ids.tolist() == [2] and ds.tolist() == [1.0]   # strict
    v = np.float32([[0.0, -0.0, np.nan, 1e-45, -1.0, np.inf, -np.inf, 0.5, 0.5]])
    assert B.from_float(v).tolist() == [[0b10101000, 0b1]]
    t = np.float32([0, 0, 0, 0, -1.0, np.inf, -np.inf, 0.5, 0.25])
    assert B.from_float(v, t).tolist() == [[0b00001000, 0b1]]                   # equal to the threshold: 0; -inf > -inf: 0


def test_argument_errors_come_before_any_device_call(lib):
    """What can be refused without a device is refused first: `fake` is never dereferenced."""
    from deltapq_amd import api
    fake = ctypes.c_void_p(0x1000)
    h = ctypes.c_void_p(0x2000)
    out = ctypes.byref(h)

    def call(name, data=fake, n=10, D=64, thr=None, off=0, out=out, res=fake):
        fn = getattr(lib, name)
        if name == "dpq_flat_open_bits":
            return fn(data, n, D, 0, off, out)
        if name == "dpq_bits_from_float":
            return fn(data, n, D, thr, 0, res)
        return fn(data, n, D, thr, 0, off, out)
    every = ("dpq_flat_open_bits", "dpq_flat_open_binarised", "dpq_bits_from_float")
    opens = every[:2]
    cases = [(every, dict(data=None), "NULL"), (opens, dict(out=None), "NULL"), (every[2:], dict(res=None), "NULL"),
             (every, dict(n=0), "n < 1"), (every, dict(n=-3), "n < 1"), (every, dict(D=0), "D outside 1..4096"),
             (every, dict(D=4097), "D outside 1..4096"), (every, dict(D=-1), "D outside 1..4096"),
             (opens, dict(off=-1), "id_offset"), (opens, dict(off=(1 << 31) - 10), "id_offset"),
             # the order: n before D before id_offset
             (every, dict(n=0, D=0, off=-1), "n < 1"), (opens, dict(D=0, off=-1), "D outside")]
    for names, kw, what in cases:
        for name in names:
            assert call(name, **kw) == -1, (name, kw)
            msg = lib.dpq_last_error()
            assert name.encode() in msg and what.encode() in msg, (name, kw, msg)
    assert h.value is None                                             # *out is cleared wherever out is given
    if api.device_count() == 0:                                        # good arguments: the device is looked for next
        for name in every:
            assert call(name) == -4, name
            assert call(name, D=4096) == -4, name                      # 4096 is allowed, beyond the other handles' 2048
        assert call("dpq_flat_open_bits", off=(1 << 31) - 11) == -4


def test_python_face_refuses_what_it_cannot_take(lib, monkeypatch):
    from deltapq_amd import _lib, api

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    ok = np.zeros((3, 2), dtype=np.uint8)
    for bad in (ok.astype(np.int8), ok.astype(np.float32), ok.astype(bool), ok.astype(np.uint16), ok.tolist()):
        with pytest.raises(TypeError):
            api.FlatIndexBits(bad, 9)
    for D in (8, 17, 3):                                               # a second dimension other than (D + 7) // 8
        with pytest.raises(ValueError):
            api.FlatIndexBits(ok, D)
    with pytest.raises(ValueError):
        api.FlatIndexBits(ok[0], 16)
    v = np.zeros((3, 9), dtype=np.float32)
    for call in (lambda: api.bits_from_float(v.astype(np.float64)), lambda: api.FlatIndexBits.from_float(v.astype(np.float16)),
                 lambda: api.bits_from_float(v, np.zeros(9, dtype=np.float64)),
                 lambda: api.FlatIndexBits.from_float(v, [0.0] * 9)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: api.bits_from_float(v[0]), lambda: api.bits_from_float(v, np.zeros(8, dtype=np.float32)),
                 lambda: api.FlatIndexBits.from_float(v, np.zeros((1, 9), dtype=np.float32))):
        with pytest.raises(ValueError):
            call()


def test_cli_refuses_hamming_over_fvecs(built):
    common = [EXE, "-dataset", "/nonexistent", "-task", "groundtruth", "-topk", "1", "-query_size", "1", "-metric", "hamming"]
    for extra in ([], ["-ext", "fvecs"]):
        r = subprocess.run(common + extra, capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.startswith("usage: -metric hamming"), r.stdout
    r = subprocess.run([EXE, "-dataset", "/nonexistent", "-task", "recall", "-ext", "bvecs", "-metric", "hamming"],
                       capture_output=True, text=True)                # no other task takes it
    assert r.returncode == 2 and r.stdout.startswith("usage: -metric hamming"), r.stdout
    r = subprocess.run([EXE, "-task", "groundtruth"], capture_output=True, text=True)
    assert r.returncode == 2 and "-metric l2|ip|hamming" in r.stdout


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
    bad_i = int((gi != wi).sum()) if gi.shape == wi.shape else -1
    bad_d = int((bits_of(gd) != bits_of(wd)).sum()) if gd.shape == wd.shape else -1
    print("%s: %d of %d ids and %d of %d float bit patterns differ" % (what, bad_i, wi.size, bad_d, wd.size))
    assert gi.shape == wi.shape and bad_i == 0 and bad_d == 0, what


def assert_same_lists(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ": lims"
    assert_same(got[1:], want[1:], what)


_cases = {}


def case(n, D, nq=65, seed=0):
    """Rows, queries (a few of them copies of rows) and their distance table, made once per shape and never changed."""
    key = (n, D, nq, seed)
    if key not in _cases:
        base = random_packed(n, D, seed=1000 * seed + n + D)
        queries = random_packed(nq, D, seed=7 + 1000 * seed + n + D, dup=0)
        queries[::4] = base[np.random.default_rng(n).integers(0, n, size=len(queries[::4]))]
        dist = B.all_distances(base, queries, D)
        for a in (base, queries, dist):
            a.setflags(write=False)
        _cases[key] = (base, queries, dist)
    return _cases[key]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 7, 8, 9, 127, 128, 129, 1000, 4096])
def test_gpu_padding_and_spare_bits(gpu, D):
    n, nq, k = 300, 5, 50
    base, queries, dist = case(n, D, nq)
    want = B.search(base, queries, D, k, dist=dist)
    want_r = B.range_search(base, queries, D, np.float32(D / 2 + 1), dist=dist)
    answers = []
    for ones in (True, False):
        with gpu.FlatIndexBits(with_spare(base, D, ones), D) as f:
            got = f.search(with_spare(queries, D, ones), k)
            got_r = f.range_search(with_spare(queries, D, not ones), np.float32(D / 2 + 1))
        assert_same(got, want, "D %d spare bits %s" % (D, "ones" if ones else "zeros"))
        assert_same_lists(got_r, want_r, "D %d range, spare bits mixed" % D)
        answers.append(got)
    assert np.array_equal(answers[0][0], answers[1][0]) and np.array_equal(bits_of(answers[0][1]), bits_of(answers[1][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 63, 64, 65])
@pytest.mark.parametrize("n,D", [(1, 72), (255, 72), (256, 72), (257, 72), (4096, 72), (4097, 72), (9000, 72), (257, 1024), (9000, 1024)])
def test_gpu_tile_and_stripe_edges(gpu, n, D, nq):
    """top_k = 100: a stripe is 4096 entries; 256 entries and 64 queries to a workgroup; rows of 16 bytes take the kernel's
    4-word form, rows of 128 bytes its 32-word form."""
    base, queries, dist = case(n, D)
    k = min(100, n)
    with gpu.FlatIndexBits(base, D) as f:
        got = f.search(queries[:nq], k)
    assert_same(got, B.search(base, queries[:nq], D, k, dist=dist[:nq]), "n %d D %d nq %d" % (n, D, nq))


@pytest.mark.gpu
def test_gpu_ties_decide_everything(gpu):
    D, n = 8, 9000                                                     # nine distinct distances
    base, queries, dist = case(n, D, 5)
    with gpu.FlatIndexBits(base, D, id_offset=11) as f:
        for k in (1, 100, 2049, 9000):
            assert_same(f.search(queries, k), B.search(base, queries, D, k, id_offset=11, dist=dist), "D 8 top_k %d" % k)
        everything = gpu.FlatIdFilter.from_mask(f, np.ones(n + 11, dtype=bool))
        got = f.search_filtered(queries, 9100, everything)            # top_k > n pads
        assert_same(got, B.search(base, queries, D, 9100, id_offset=11, dist=dist), "top_k above n")
        assert (got[0][:, 9000:] == -1).all() and np.isinf(got[1][:, 9000:]).all()
        with pytest.raises(gpu.DpqError) as e:
            f.search(queries, 9001)
        assert e.value.status == -8                                    # DPQ_ERR_TOPK on the plain call
    base, queries, dist = case(20000, 16, 3)
    with gpu.FlatIndexBits(base, 16) as f:
        assert_same(f.search(queries, 4096), B.search(base, queries, 16, 4096, dist=dist), "n 20000 D 16 top_k 4096")
    D, n = 200, 5000                                                   # all rows equal to the query
    row = random_packed(1, D, seed=5)
    base = np.repeat(row, n, axis=0)
    with gpu.FlatIndexBits(base, D) as f:
        i, d = f.search(row, 100)
        assert i.tolist() == [list(range(100))] and not d.any()
        lims, ids, ds = f.range_search(row, 1.0)
        assert lims.tolist() == [0, n] and ids.tolist() == list(range(n)) and not ds.any()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 1000, 2048])
def test_gpu_byte_handle_over_the_unpacked_rows_agrees(gpu, D):
    """An independent yardstick on the device: squared L2 of 0/1 bytes on the int8 matrix cores is the Hamming distance."""
    n, nq, k = 3000, 8, 100
    base, queries, dist = case(n, D, nq)
    b01, q01 = B.unpack_bits(base, D), B.unpack_bits(queries, D)
    mask = np.random.default_rng(D).random(n + 5) < 0.3
    radii = np.sort(dist, axis=1)[:, 40].astype(np.float32) + np.float32([0, 1] * (nq // 2))
    with gpu.FlatIndexBits(base, D, id_offset=5) as f, gpu.FlatIndexU8(b01, id_offset=5) as u:
        assert_same(f.search(queries, k), u.search(q01, k), "search D %d" % D)
        ff, uf = gpu.FlatIdFilter.from_mask(f, mask), gpu.FlatIdFilter.from_mask(u, mask)
        assert_same(f.search_filtered(queries, k, ff), u.search_filtered(q01, k, uf), "filtered D %d" % D)
        assert_same_lists(f.range_search(queries, radii), u.range_search(q01, radii), "range D %d" % D)
        assert_same_lists(f.range_search(queries, radii, ff), u.range_search(q01, radii, uf), "filtered range D %d" % D)


@pytest.mark.gpu
def test_gpu_filtered(gpu):
    n, D, nq, k, off = 9000, 136, 9, 100, 7
    base, queries, dist = case(n, D, nq)
    rng = np.random.default_rng(3)
    one = np.zeros(n + off, dtype=bool)
    one[off + 4321] = True
    masks = {"50 % (the list crosses a stripe)": rng.random(n + off) < 0.5, "1 %": rng.random(n + off) < 0.01, "one row": one,
             "empty": np.zeros(n + off, dtype=bool), "short bitmap": np.ones(off + 100, dtype=bool)}
    assert masks["50 % (the list crosses a stripe)"][off:].sum() > 4096
    with gpu.FlatIndexBits(base, D, id_offset=off) as f:
        for what, mask in masks.items():
            allowed = B.allowed_rows(n, off, mask)
            with gpu.FlatIdFilter.from_mask(f, mask) as ff:
                assert ff.n_allowed == int(allowed.sum())
                assert_same(f.search_filtered(queries, k, ff), B.search(base, queries, D, k, id_offset=off, allowed=allowed, dist=dist),
                            "filter " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
def test_gpu_range(gpu, filtered):
    n, D, nq, off = 5000, 40, 12, 7
    base, queries, dist = case(n, D, nq)
    assert (dist == 0).any()                                           # exact matches exist: radius 1 finds them, 0 nothing
    mask = np.random.default_rng(9).random(n + off) < 0.4
    allowed = B.allowed_rows(n, off, mask) if filtered else None
    per_query = np.float32([0, 0.5, 1, 3, 10, 17.5, 20, 21, 25, D, D + 1, np.inf])
    with gpu.FlatIndexBits(base, D, id_offset=off) as f:
        ff = gpu.FlatIdFilter.from_mask(f, mask) if filtered else None
        for r in (0.0, 0.5, 1.0, 18.0, float(D), float(D + 1), np.inf, per_query):
            got = f.range_search(queries, r, ff)
            want = B.range_search(base, queries, D, r, id_offset=off, allowed=allowed, dist=dist)
            assert_same_lists(got, want, "radius %s filtered %s" % (r if np.isscalar(r) else "per query", filtered))
        assert f.range_search(queries, 0.0, ff)[0][-1] == 0 and f.range_search(queries, 0.5, ff)[0][-1] > 0
        everything = f.range_search(queries, np.inf, ff)
        assert everything[0][-1] == nq * (n if allowed is None else int(allowed.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [72, 1000])
def test_gpu_range_with_the_wide_query_tile(gpu, D):
    """A pass of more than 256 tiles of 256 entries x 64 queries takes the distance kernel's 32-query form (a top-k stripe
    and every smaller pass its 16-query form), with and without a row list, at both row lengths."""
    n, nq = 4400, 961                                                  # 18 x 16 tiles; 17 x 16 under the filter
    base, queries, dist = case(n, D, nq)
    mask = np.random.default_rng(D).random(n) < 0.97
    assert mask.sum() > 4096
    radii = np.sort(dist, axis=1)[:, 25].astype(np.float32) + np.float32(1)
    with gpu.FlatIndexBits(base, D) as f:
        assert_same_lists(f.range_search(queries, radii), B.range_search(base, queries, D, radii, dist=dist), "wide tile D %d" % D)
        with gpu.FlatIdFilter.from_mask(f, mask) as ff:
            assert_same_lists(f.range_search(queries, radii, ff), B.range_search(base, queries, D, radii, allowed=mask, dist=dist),
                              "wide tile, filtered, D %d" % D)


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n_cand", [1, 100, 1000])
def test_gpu_rerank_host_and_device(gpu, n_cand, mapped):
    import torch
    n, D, nq, off = 3000, 130, 7, 0 if mapped else 9                   # an even-N map
    base, queries, _ = case(n, D, nq)
    rng = np.random.default_rng(n_cand)
    id_map = rng.permutation(n).astype(np.uint32) if mapped else None
    hi = n + 1 if mapped else n                                        # with the map, candidate n names the last position
    cand = (rng.integers(0, hi, size=(nq, n_cand)) + (0 if mapped else off)).astype(np.int32)
    if n_cand > 1:
        cand[:, ::7] = -1                                              # padding candidates
        cand[:, 1::5] = cand[:, 2:3]                                   # repeated candidates
        cand[0, :] = -1                                                # a query with nothing but padding
    if mapped:
        cand[-1, -1] = n
    k = min(n_cand, 50)
    want = B.rerank(base, queries, D, cand, k, id_offset=off, id_map=id_map)
    with gpu.FlatIndexBits(with_spare(base, D, True), D, id_offset=off) as f:
        if mapped:
            f.set_id_map(id_map)
        assert_same(f.rerank(with_spare(queries, D, True), cand, k), want, "host n_cand %d" % n_cand)
        tq, tc = torch.from_numpy(with_spare(queries, D, True)).cuda(), torch.from_numpy(cand).cuda()
        ti, td = f.rerank_torch(tq, tc, k)
        assert_same((ti.cpu().numpy(), td.cpu().numpy()), want, "device n_cand %d" % n_cand)
        bad = cand.copy()
        bad[-1, 0] = (n + 1 if mapped else n + off)                    # names no row
        for call in (lambda: f.rerank(queries, bad, k), lambda: f.rerank_torch(tq, torch.from_numpy(bad).cuda(), k)):
            with pytest.raises(gpu.DpqError) as e:
                call()
            assert e.value.status == -1 and "names no row" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 9, 130])
def test_gpu_bits_from_float(gpu, D):
    n, nq = 700, 6
    rng = np.random.default_rng(D)
    v = rng.standard_normal((n, D)).astype(np.float32)
    t = rng.standard_normal(D).astype(np.float32)
    special = np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45])
    v[rng.integers(0, n, size=200), rng.integers(0, D, size=200)] = special[rng.integers(0, len(special), size=200)]
    rows = rng.integers(0, n, size=100)
    v[rows, rng.integers(0, D, size=100)] = 0.0
    cols = rng.integers(0, D, size=100)
    v[rows, cols] = t[cols]                                            # values equal to their threshold
    if D > 1:
        t[1] = np.inf
    queries = random_packed(nq, D, seed=D, dup=0)
    for thr in (None, t):
        want = B.from_float(v, thr)
        got = gpu.bits_from_float(v, thr)
        bad = int((got != want).sum())
        print("D %d thresholds %s: %d of %d bytes differ" % (D, "given" if thr is not None else "none", bad, want.size))
        assert got.dtype == np.uint8 and got.shape == want.shape and bad == 0
        with gpu.FlatIndexBits.from_float(v, thr, id_offset=4) as a, gpu.FlatIndexBits(want, D, id_offset=4) as b:
            assert (a.n, a.D) == (n, D)
            assert_same(a.search(queries, 60), b.search(queries, 60), "from_float against the handle over its bytes")
            assert_same(a.search(queries, 60), B.search(want, queries, D, 60, id_offset=4), "from_float against the restatement")


@pytest.mark.gpu
def test_gpu_handle_kinds(gpu, lib):
    D = 64
    q8, qf = np.zeros((2, D), dtype=np.uint8), np.zeros((2, D), dtype=np.float32)
    i, s = np.empty((2, 4), dtype=np.int32), np.empty((2, 4), dtype=np.float32)
    c = np.zeros((2, 4), dtype=np.int32)
    r = np.ones(2, dtype=np.float32)
    res = ctypes.c_void_p()
    with gpu.FlatIndexBits(np.zeros((70, D // 8), dtype=np.uint8), D) as f, gpu.FlatIndexU8(np.zeros((70, 8), dtype=np.uint8)) as u, \
            gpu.FlatIndex(np.zeros((70, 8), dtype=np.float32)) as x:
        ff = gpu.FlatIdFilter.from_mask(f, np.ones(70, dtype=bool))
        for kind, q in (("", qf), ("_ip", qf), ("_u8", q8), ("_ip_u8", q8), ("_i8", q8), ("_ip_i8", q8)):
            calls = {"dpq_flat_search" + kind: lambda fn: fn(f._h, p(q), 2, 4, p(i), p(s)),
                     "dpq_flat_search_filtered" + kind: lambda fn: fn(f._h, ff._h, p(q), 2, 4, p(i), p(s)),
                     "dpq_flat_range_search" + kind: lambda fn: fn(f._h, None, p(q), 2, p(r), ctypes.byref(res)),
                     "dpq_flat_rerank" + kind: lambda fn: fn(f._h, p(q), 2, p(c), 4, 4, p(i), p(s)),
                     "dpq_flat_rerank%s_device" % kind: lambda fn: fn(f._h, p(q), 2, p(c), 4, 4, p(i), p(s), None)}
            for name, call in calls.items():
                assert call(getattr(lib, name)) == -1, name
                msg = lib.dpq_last_error()
                right = name.replace(kind, "_bits", 1) if kind else name.replace("_device", "") + "_bits" + ("_device" if "_device" in name else "")
                assert name.encode() in msg and b"binary vectors" in msg and msg.endswith(b"call " + right.encode()), msg
        for m in (f.search_ip, lambda q, k: f.search_filtered_ip(q, k, ff), lambda q, k: f.range_search_ip(q, 1.0),
                  lambda q, k: f.rerank_ip(q, np.zeros((2, 4), dtype=np.int32), k)):
            with pytest.raises(gpu.DpqError) as e:
                m(np.zeros((2, D // 8), dtype=np.uint8), 4)
            assert e.value.status == -1 and "_bits" in str(e.value)
        assert lib.dpq_flat_search_bits(u._h, p(q8), 2, 4, p(i), p(s)) == -1   # a _bits call on any other handle
        assert b"dpq_flat_search_bits: the handle holds byte vectors (dpq_flat_open_u8); call dpq_flat_search_u8" in lib.dpq_last_error()
        assert lib.dpq_flat_rerank_bits(x._h, p(q8), 2, p(c), 4, 4, p(i), p(s)) == -1
        assert b"dpq_flat_rerank_bits: the handle holds fp32 vectors (dpq_flat_open); call dpq_flat_rerank" in lib.dpq_last_error()
        assert lib.dpq_flat_search_u8(x._h, p(q8), 2, 4, p(i), p(s)) == -1       # the other kinds answer as before
        assert b"the handle holds fp32 vectors (dpq_flat_open); call dpq_flat_search" in lib.dpq_last_error()
        assert f.search(np.zeros((2, D // 8), dtype=np.uint8), 4)[0].tolist() == [[0, 1, 2, 3]] * 2


@pytest.mark.gpu
def test_gpu_cli_groundtruth_hamming(gpu, tmp_path):
    from deltapq_amd import synth
    n, nb, nq, k = 3000, 16, 20, 10
    D = 8 * nb
    base, queries, dist = case(n, D, nq)
    d = str(tmp_path)
    synth.write_bvecs(os.path.join(d, "base.bvecs"), base)
    synth.write_bvecs(os.path.join(d, "query.bvecs"), queries)
    common = [EXE, "-dataset", d, "-task", "groundtruth", "-topk", str(k), "-query_size", str(nq), "-ext", "bvecs", "-metric", "hamming"]
    env = dict(os.environ, DPQ_DEV="1", DPQ_GT_PART_ROWS="1100")       # three slices, merged on the host
    r = subprocess.run(common, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "3 part(s)" in r.stdout, r.stdout + r.stderr
    got = gpu.read_groundtruth(os.path.join(d, "groundtruth", "N%dTop%d.hamming.txt" % (n, k)))
    assert_same(got, B.search(base, queries, D, k, dist=dist), "cli")
    mask = np.random.default_rng(1).random(n) < 0.2
    gpu.write_bitmap(os.path.join(d, "filter.bin"), *gpu.FlatIdFilter.pack_mask(mask))
    r = subprocess.run(common + ["-filter", os.path.join(d, "filter.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = gpu.read_groundtruth(os.path.join(d, "groundtruth", "N%dTop%d.hamming.filtered.txt" % (n, k)))
    assert_same(got, B.search(base, queries, D, k, allowed=mask, dist=dist), "cli -filter")
