"""The codebook trainer at its edges: dpq_train.hip through dpq_train_codebook, dpq_kmeanspp_seed and dpq_train_potential.

Every width of train_assign_kernel, the second upload tile and the second chunk of leaf sums, winning distances that
overflow, and the corners of the argument range (M = 256, the largest shapes the LDS check accepts, n == K, a ragged
block of one vector, sub-spaces that are nothing but padding, sub-spaces that stop rounds apart).

The rules are this build's own (include/deltapq_amd.h), restated on the CPU in
tests/_kmeans_restatement.py and tests/_kmeanspp_restatement.py; the GPU has to meet them bit for bit, with no tolerance
anywhere.  One table of cases serves both sides: on the CPU every case is shown to reach what its name claims, on the GPU
the kernels have to give the restatement's bits."""
import ctypes
import functools

import numpy as np
import pytest

import _kmeans_restatement as R
import _kmeanspp_restatement as P
from oracle import pq_encode_oracle as E
from test_train_kmeanspp import case as seeding_case            # the `binades` case and its restated seeding

ERR_ARG, ERR_NO_DEVICE = -1, -4
WIDTHS = [4, 8, 12, 16, 24, 32, 64, 96, 128, 160]    # the padded widths train_assign_kernel is compiled for, literally
LDS_LIMIT = 160 * 1024
LEAF, CHUNK, UPLOAD = 256, 1024, 1 << 18             # vectors per leaf, leaf sums per LDS chunk, vectors per upload


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def padded(Ds):
    return next(w for w in WIDTHS if Ds <= w)


def vectors_per_thread(Ds):
    return 2 if padded(Ds) <= 32 else 1


def assign_blocks(n, Ds):
    return -(-n // (256 * vectors_per_thread(Ds)))


def lds_bytes(K, Ds):
    """The dynamic LDS of one assignment block: the codewords, a 256-entry histogram, four fp64 and four u32 partials."""
    return K * padded(Ds) * 4 + 256 * 4 + 4 * 8 + 4 * 4


def spread(rng, n, D):
    """Normal values over six decades, as test_train_codebook's b_real: the small terms of a distance vanish or survive
    with the order of the fp32 adds, so only the in-order sum gives the stated distances."""
    return (rng.normal(size=(n, D)) * 10.0 ** rng.uniform(-3, 3, size=(n, D))).astype(np.float32)


def assert_sums_exact_in_any_order(wins):
    """Every winning distance of a round is a multiple of one power of two q, and their sum is below 2**52 * q: every
    partial sum, in whatever order, is then a multiple of q below 2**53 * q, an fp64 number, and no add rounds."""
    for r, w in enumerate(wins):
        w = np.asarray(w, dtype=np.float64).ravel()
        total = float(w.sum())
        assert np.isfinite(total) and total > 0
        q = 2.0 ** (int(np.ceil(np.log2(total))) + 1 - 52)
        assert np.array_equal(w / q, np.floor(w / q)), "round %d: a distance is no multiple of %g" % (r + 1, q)


# ---- A: every width of the assignment --------------------------------------------------------------------------------

WIDTH_DS = [3, 4, 5, 11, 12, 16, 23, 24, 32, 33, 96, 127, 128, 129, 160]
WIDTH_N = 777                                        # two blocks of 512 with a ragged tail, or four of 256
SEEDED_WIDTHS = (12, 32, 160)                        # where the k-means++ seeding runs too


@functools.lru_cache(maxsize=None)
def width_case(Ds):
    """(case, restated codebook, restated stats, restated potential, restated seeding or None)."""
    c = dict(vectors=spread(np.random.default_rng(1000 + Ds), WIDTH_N, 2 * Ds), M=2, K=32, max_iters=3, seed=Ds)
    cb, st = R.train(c["vectors"], c["M"], c["K"], c["max_iters"], c["seed"])
    seeded = P.kmeanspp_seed(c["vectors"], c["M"], c["K"], c["seed"]) if padded(Ds) in SEEDED_WIDTHS else None
    return c, cb, st, P.potential(c["vectors"], cb), seeded


def test_width_cases_reach_all_ten_instances():
    assert sorted({padded(Ds) for Ds in WIDTH_DS}) == [4, 8, 12, 16, 24, 32, 64, 96, 128, 160]
    below = {padded(Ds) for Ds in WIDTH_DS if Ds < padded(Ds)}
    at = {Ds for Ds in WIDTH_DS if Ds == padded(Ds)}
    assert below >= {4, 8, 12, 24, 64, 128, 160} and at >= {4, 12, 16, 24, 32, 96, 128, 160}
    assert {padded(Ds) for Ds in WIDTH_DS if padded(Ds) in SEEDED_WIDTHS} == set(SEEDED_WIDTHS)
    assert padded(160) // 4 == 40                    # the seeding's centre load: 40 lanes of float4
    for Ds in WIDTH_DS:                              # more than one block, and the last one ragged
        per_block = 256 * vectors_per_thread(Ds)
        assert assign_blocks(WIDTH_N, Ds) == (2 if Ds <= 32 else 4) and WIDTH_N % per_block not in (0, 1)
        assert lds_bytes(32, Ds) <= LDS_LIMIT


def test_width_cases_depend_on_the_order_of_the_fp32_sum():
    """The same distances summed in fp64 and rounded once differ from the in-order fp32 sum in their bits."""
    for Ds in (12, 33, 160):
        c, cb, _, _, _ = width_case(Ds)
        sub = R.split(c["vectors"], 2)[0]
        _, win = R.assign(sub, cb[0])
        wide = ((sub.astype(np.float64)[:, None, :] - cb[0].astype(np.float64)[None]) ** 2).sum(2).min(1).astype(np.float32)
        assert (bits(win) != bits(wide)).sum() >= WIDTH_N // 10


# ---- B: past 2**18 vectors -------------------------------------------------------------------------------------------

PAST_N = 1025 * LEAF + 1                             # a second upload of 257 vectors; leaf 1025 holds one vector
PAST_MARKED = {UPLOAD - 1: (1, 2), UPLOAD: (2, 3), UPLOAD + 1: (3, 1)}      # vector -> its labels, by construction
PAST_SEED = 1                                        # of the seeding, searched: see test_past_upload_case_...


def _past_vectors():
    """Integers 0..9, K = 4 codewords per sub-space: (5, 5) and (100 k, 100 k), k = 1..3.  The three vectors around the
    upload boundary ARE codewords 1..3, each of another pair, and no other vector comes near them: a base that is off
    by one empties a cluster and moves a mean.  The last vector, alone in leaf 1025, is far from everything: round 1
    puts it with codeword 3, whose mean it drags away from the one sub-vector at 255, which changes sides in round 2,
    so that a third round runs."""
    v = np.random.default_rng(7).integers(0, 10, size=(PAST_N, 4)).astype(np.float32)
    for i, (a, b) in PAST_MARKED.items():
        v[i] = (100 * a, 100 * a, 100 * b, 100 * b)
    v[PAST_N - 1] = 400
    v[1000, :2] = 255
    v[200000, 2:] = 255
    init = np.array([[[5, 5], [100, 100], [200, 200], [300, 300]]] * 2, dtype=np.float32)
    return v, init


@functools.lru_cache(maxsize=None)
def past_case():
    v, init = _past_vectors()
    c = dict(vectors=v, M=2, K=4, max_iters=3, seed=0, init=init)
    cb, st = R.train(v, 2, 4, 3, 0, init)
    return c, cb, st, P.potential(v, cb), P.kmeanspp_seed(v, 2, 4, PAST_SEED)


def test_past_upload_case_reaches_the_second_tile_and_the_second_chunk():
    c, cb, st, pot, (seeded, seed_pot, info) = past_case()
    v = c["vectors"]
    assert PAST_N - UPLOAD == 257 and -(-PAST_N // LEAF) == CHUNK + 2 and PAST_N - (CHUNK + 1) * LEAF == 1
    assert PAST_N * c["M"] * 4 < 2 ** 31
    # the marked vectors keep the labels they were built for, so each is a cluster of its own around the boundary
    for i, want in PAST_MARKED.items():
        assert tuple(st["labels"][i]) == want
    # ... and a second tile written one vector early or late (one vector overwritten or left out) gives another codebook
    early, late = v.copy(), v.copy()
    early[UPLOAD - 1:-1], early[-1] = v[UPLOAD:], 0
    late[UPLOAD + 1:], late[UPLOAD] = v[UPLOAD:-1], 0
    for off in (early, late):
        assert not np.array_equal(bits(R.train(off, 2, 4, 3, 0, c["init"])[0]), bits(cb))
    assert_sums_exact_in_any_order(st["wins"])
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (3, 1, 0)
    assert [int((a != b).any()) for a, b in zip(st["wins"][:-1], st["wins"][1:])] == [1, 1]    # every round moved something
    # the seeding: a draw whose r lies beyond T[1023], so the running total carried into the second chunk decides it,
    # and one that takes the last leaf, the one vector of leaf 1025
    drawn = [row for rows in info["rows"] for row in rows[1:]]
    assert any(row // LEAF >= CHUNK for row in drawn), drawn
    assert PAST_N - 1 in drawn, drawn
    assert all(h == "walk" for how in info["how"] for h in how)


# ---- C: winning distances that overflow ------------------------------------------------------------------------------

def potential_from_flt_max(vectors, codebook):
    """What a search that reports its starting value would give: FLT_MAX where no distance is below FLT_MAX."""
    out = []
    for m, sub in enumerate(R.split(vectors, len(codebook))):
        _, win = R.assign(sub, np.asarray(codebook[m], dtype=np.float32))
        out.append(P.potential_of_weights(np.where(win < E.FLT_MAX, win, E.FLT_MAX).astype(np.float32)))
    return np.array(out)


def test_binades_potential_is_infinite_where_every_distance_overflows():
    c, seeded, seed_pot, _ = seeding_case("binades")
    pot = P.potential(c["vectors"], seeded)
    assert np.isfinite(pot[0]) and pot[1] == np.inf
    assert np.array_equal(bits64(pot), bits64(seed_pot))               # the seeding's weights are those distances
    sub = R.split(c["vectors"], 2)[1]
    dist = E.sub_distances(c["vectors"], seeded, 1)
    lost = np.isinf(dist).all(1)
    lab, win = R.assign(sub, seeded[1])
    assert lost.sum() >= 2 and not lab[lost].any() and np.isinf(win[lost]).all() and np.isfinite(win[~lost]).all()
    assert np.array_equal(lab, E.encode_pq(c["vectors"], seeded)[:, 1])
    assert np.isfinite(potential_from_flt_max(c["vectors"], seeded)).all()     # the number FLT_MAX would make of it


RESTART_ROWS = (37, 150, 271)
RESTART_SEED = 2                                     # see test_restart_case_...


def _restart_case(seed=None):
    """300 rows, M = 2.  Sub-space 1 lives at 2**50, so its finite potential is around 2**110, and three of its rows sit
    at 2**65 in three different quadrants: the distance of each to every other row, and to any mean it is part of,
    is beyond fp32.  K = 4 and the rows start: no run makes a centre of all three."""
    v = np.random.default_rng(31).normal(size=(300, 4)).astype(np.float32)
    v[:, 2:] *= np.float32(2.0 ** 50)
    big = np.float32(2.0 ** 65)
    for row, signs in zip(RESTART_ROWS, ((1, 1), (-1, 1), (1, -1))):
        v[row, 2:] = big * np.array(signs, dtype=np.float32)
    return dict(vectors=v, M=2, K=4, max_iters=4, seed=RESTART_SEED if seed is None else seed, restarts=3)


@functools.lru_cache(maxsize=None)
def restart_case():
    c = _restart_case()
    return c, P.train(**c)


def restart_properties(c, cb, st):
    """(every run's potential of sub-space 1 is +inf, what FLT_MAX in its place would have kept, whether that differs)."""
    pots = np.array([p[1] for _, _, p in st["runs"]])
    finite = np.array([potential_from_flt_max(c["vectors"], run_cb)[1] for run_cb, _, _ in st["runs"]])
    other = int(finite.argmin())
    differs = not np.array_equal(bits(st["runs"][other][0][1]), bits(st["runs"][0][0][1]))
    return bool(np.isinf(pots).all()), other, differs, finite


def test_restart_case_ties_at_infinity_where_flt_max_would_order_the_runs():
    c, (cb, st) = restart_case()
    all_inf, other, differs, finite = restart_properties(c, cb, st)
    print("potentials with FLT_MAX for +inf:", finite.tolist(), "kept then: run", other)
    sub = R.split(c["vectors"], 2)[1]
    for row in RESTART_ROWS:                                           # beyond fp32 from every other row
        assert np.isinf(R.assign(np.delete(sub, row, axis=0), sub[row:row + 1])[1]).all()
    assert all_inf and st["winner"][1] == 0                            # the contract: a tie, the lowest r is kept
    assert np.isfinite(finite).all() and other != 0 and differs        # what lets the GPU test see the difference
    assert np.array_equal(bits(cb[1]), bits(st["runs"][0][0][1]))
    assert st["distortion"][0] == np.inf


def _flt_max_pair():
    """(x, y) with fl(fl(x * x) + fl(y * y)) == FLT_MAX exactly, or None: x = 2**63 (1 + i 2**-23), y from the square
    root of what is missing, a few neighbours tried."""
    for i in range(4096):
        x = np.float32(2.0 ** 63 * (1 + i * 2.0 ** -23))
        p = np.float32(x * x)
        y0 = np.float32(np.sqrt(np.float64(E.FLT_MAX) - np.float64(p)))
        for step in range(-2, 3):
            y = (y0.view(np.uint32) + np.uint32(step)).view(np.float32) if step >= 0 else \
                (y0.view(np.uint32) - np.uint32(-step)).view(np.float32)
            with np.errstate(over="ignore"):
                if np.float32(p + np.float32(y * y)) == E.FLT_MAX:
                    return float(x), float(y)
    return None


@functools.lru_cache(maxsize=None)
def flt_max_case():
    """M = 1, Ds = 2, K = 2: codeword 0 is beyond fp32 from every vector, codeword 1 is the origin.  Vector 0 is exactly
    FLT_MAX from the origin: not below FLT_MAX, so its label is the encoder's 0 and its winning distance +inf, where an
    argmin would say label 1 at FLT_MAX.  The other vectors are small and take label 1."""
    x, y = _flt_max_pair()
    v = np.array([[x, y], [1, 2], [3, -1], [-2, 2], [0, 1]], dtype=np.float32)
    init = np.array([[[-3e19, -3e19], [0, 0]]], dtype=np.float32)
    return dict(vectors=v, M=1, K=2, max_iters=1, seed=0, init=init)


def test_flt_max_case_is_exactly_flt_max_behind_an_infinite_codeword_0():
    assert _flt_max_pair() is not None
    c = flt_max_case()
    dist = E.sub_distances(c["vectors"], c["init"], 0)
    assert dist[0, 0] == np.inf and dist[0, 1] == E.FLT_MAX and dist[0].argmin() == 1
    lab, win = R.assign(c["vectors"], c["init"][0])
    assert lab.tolist() == [0, 1, 1, 1, 1] and win[0] == np.inf and np.isfinite(win[1:]).all()
    assert E.encode_pq(c["vectors"], c["init"])[:, 0].tolist() == lab.tolist()
    cb, st = R.train(**c)
    assert np.array_equal(cb[0, 0], c["vectors"][0]) and st["distortion"] == [np.inf]     # cluster 0 is vector 0 alone


# ---- D: the corners --------------------------------------------------------------------------------------------------

def _corner_m256():          # key_bits = 16, and (m = 255, k = 255) is the key 0xFFFF the key array is pre-filled with
    v = np.random.default_rng(41).integers(0, 200, size=(300, 256)).astype(np.float32)
    return dict(vectors=v, M=256, K=256, max_iters=3, seed=2, init=None)


def _corner_lds_k254_ds160():   # the largest accepted shape at Ds = 129..160: 163 632 of 163 840 bytes
    return dict(vectors=spread(np.random.default_rng(42), 600, 320), M=2, K=254, max_iters=2, seed=3, init=None)


def _corner_lds_k256_ds128():   # the largest accepted shape at K = 256: 132 144 bytes
    return dict(vectors=spread(np.random.default_rng(43), 600, 256), M=2, K=256, max_iters=2, seed=4, init=None)


def _corner_n_equals_k():       # the rows start makes every vector a cluster of its own
    return dict(vectors=np.random.default_rng(44).normal(size=(16, 8)).astype(np.float32), M=2, K=16, max_iters=25, seed=5,
                init=None)


def _corner_block_plus_one_v2():   # two vectors per thread: 513 = one block of 512 and a block of one vector
    return dict(vectors=spread(np.random.default_rng(45), 513, 8), M=2, K=8, max_iters=3, seed=6, init=None)


def _corner_block_plus_one_v1():   # one vector per thread (Ds = 33): 257 = one block of 256 and a block of one vector
    return dict(vectors=spread(np.random.default_rng(46), 257, 66), M=2, K=8, max_iters=3, seed=7, init=None)


def _corner_all_padding():      # D = 9, M = 8: Ds = 2, sub-space 4 half padding, sub-spaces 5..7 nothing but zeros
    return dict(vectors=np.random.default_rng(47).normal(size=(500, 9)).astype(np.float32), M=8, K=4, max_iters=4, seed=1,
                init=None)


STAGGER_K = 8


def _corner_staggered_stop():
    """Sub-space 0: eight integer points far apart, each repeated 125 times, and those points as the start: round 1
    changes nothing but the labels' first values, round 2 stops it.  Sub-space 1: integers 0..29 in two dimensions from
    its first eight rows, which takes rounds more.  Integer vectors throughout."""
    rng = np.random.default_rng(48)
    n = 1000
    points = 20.0 * np.arange(STAGGER_K)[:, None] * np.ones((1, 2))
    v = np.empty((n, 4), dtype=np.float32)
    v[:, :2] = points[np.arange(n) % STAGGER_K]
    v[:, 2:] = rng.integers(0, 30, size=(n, 2))
    init = np.stack([points, v[:STAGGER_K, 2:]]).astype(np.float32)
    return dict(vectors=v, M=2, K=STAGGER_K, max_iters=40, seed=0, init=init)


CORNERS = {f.__name__[8:]: f for f in (_corner_m256, _corner_lds_k254_ds160, _corner_lds_k256_ds128, _corner_n_equals_k,
                                        _corner_block_plus_one_v2, _corner_block_plus_one_v1, _corner_all_padding,
                                        _corner_staggered_stop)}
EXACT_TRACE = ("m256", "staggered_stop")             # integer vectors: the distortion trace is compared exactly


@functools.lru_cache(maxsize=None)
def corner(name):
    c = CORNERS[name]()
    cb, st = R.train(c["vectors"], c["M"], c["K"], c["max_iters"], c["seed"], c["init"])
    return c, cb, st


def stop_rounds(st, M):
    """Per sub-space the round (1-based) whose assignment stopped it, or None."""
    return [next((r + 1 for r, act in enumerate(st["active"]) if not act[m]), None) for m in range(M)]


def test_every_corner_reaches_what_its_name_claims():
    c, cb, st = corner("m256")
    assert c["M"] * 256 == 1 << 16 and ((255 << 8) | 255) == 0xFFFF
    first, _ = R.assign(R.split(c["vectors"], 256)[255], R.split(c["vectors"], 256)[255][R.seeded_rows(300, 256, c["seed"])])
    assert (first == 255).any() and (st["labels"][:, 255] == 255).any()       # the pre-filled key is a label in use
    assert st["reseeded"] > 0 and cb.shape == (256, 256, 1)                    # repeats: empty clusters to repair
    assert_sums_exact_in_any_order(st["wins"])

    for name, K, Ds, want in (("lds_k254_ds160", 254, 160, 163632), ("lds_k256_ds128", 256, 128, 132144)):
        c, cb, st = corner(name)
        assert cb.shape == (2, K, Ds) and lds_bytes(K, Ds) == want <= LDS_LIMIT
        assert st["iters_run"] == 2
    assert lds_bytes(255, 160) == 164272 > LDS_LIMIT and lds_bytes(255, 129) > LDS_LIMIT

    c, cb, st = corner("n_equals_k")
    assert len(c["vectors"]) == c["K"]
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (2, 1, 0)
    for m, sub in enumerate(R.split(c["vectors"], 2)):
        assert sorted(map(bytes, bits(cb[m]))) == sorted(map(bytes, bits(sub)))   # every vector is a codeword
    assert st["distortion"] == [0.0, 0.0]

    for name, Ds in (("block_plus_one_v2", 4), ("block_plus_one_v1", 33)):
        c, cb, st = corner(name)
        n = len(c["vectors"])
        assert cb.shape[2] == Ds and n % (256 * vectors_per_thread(Ds)) == 1 and assign_blocks(n, Ds) == 2

    c, cb, st = corner("all_padding")
    subs = R.split(c["vectors"], 8)
    assert cb.shape == (8, 4, 2) and subs[4][:, 0].any() and not subs[4][:, 1].any()
    assert not any(s.any() for s in subs[5:]) and not cb[5:].any()
    assert st["converged"] == 0 and st["iters_run"] == 4
    assert st["reseeded"] >= 3 * 3 * 4               # three sub-spaces with three empty clusters in each of four rounds
    assert all(act[5] and act[6] and act[7] for act in st["active"])   # all labels 0, K - 1 empty: it never stops

    c, cb, st = corner("staggered_stop")
    stops = stop_rounds(st, 2)
    print("staggered_stop: the sub-spaces stop after rounds", stops)
    assert stops[0] == 2 and stops[1] is not None and stops[1] - stops[0] >= 3
    assert st["converged"] == 1 and st["iters_run"] == stops[1] < c["max_iters"]
    assert np.array_equal(bits(cb[0]), bits(c["init"][0]))
    assert_sums_exact_in_any_order(st["wins"])


def _raw(lib, call, v, M, K):
    from deltapq_amd import _lib
    n, D = v.shape
    Ds = -(-D // M)
    cb = np.zeros((M, K, Ds), dtype=np.float32)
    pot = np.zeros(M, dtype=np.float64)
    vp, cp, pp = (ctypes.c_void_p(a.ctypes.data) for a in (v, cb, pot))
    if call == "train":
        return lib.dpq_train_codebook(vp, n, D, M, K, _lib.TrainOpts(device=0, max_iters=1, seed=0), cp, None)
    if call == "seed":
        return lib.dpq_kmeanspp_seed(vp, n, D, M, K, 0, 0, cp, pp)
    return lib.dpq_train_potential(vp, n, D, cp, M, K, Ds, 0, pp)


def test_lds_limit_errors_come_before_any_device_call(lib):
    for call in ("train", "seed", "potential"):
        for D, K in ((160, 255), (129, 255), (160, 256), (161, 2)):
            assert _raw(lib, call, np.zeros((300, D), dtype=np.float32), 1, K) == ERR_ARG, (call, D, K)
            assert b"LDS" in lib.dpq_last_error()
        for D, K in ((160, 254), (129, 254), (128, 256)):       # accepted: the call gets as far as the device
            assert _raw(lib, call, np.zeros((300, D), dtype=np.float32), 1, K) in (0, ERR_NO_DEVICE), (call, D, K)
        assert _raw(lib, call, np.zeros((300, 256), dtype=np.float32), 257, 16) == ERR_ARG       # M > 256


# ---- GPU -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def _gpu_train(gpu, c, **kw):
    return gpu.train_codebook(c["vectors"], M=c["M"], K=c["K"], max_iters=c["max_iters"], seed=c["seed"], init=c.get("init"),
                              **kw)


def assert_run_equals(what, got, want):
    (cb, st), (ref_cb, ref) = got, want
    print(what, "gpu", st["iters_run"], st["converged"], st["reseeded"], "restatement", ref["iters_run"], ref["converged"],
          ref["reseeded"])
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (ref["iters_run"], ref["converged"], ref["reseeded"])
    differing = int((bits(cb) != bits(ref_cb)).sum())
    assert differing == 0, "%s: %d of %d codeword values differ from the restatement" % (what, differing, cb.size)


def assert_seeding_equals(what, got, want):
    (cb, pot), (ref_cb, ref_pot, _) = got, want
    print(what, "seeding potential gpu", pot.tolist(), "restatement", ref_pot.tolist())
    wrong = [(m, j) for m in range(len(cb)) for j in range(cb.shape[1]) if not np.array_equal(bits(cb[m, j]), bits(ref_cb[m, j]))]
    assert not wrong, "%s: centres %s differ from the restatement" % (what, wrong[:4])
    assert np.array_equal(bits64(pot), bits64(ref_pot))


@pytest.mark.gpu
@pytest.mark.parametrize("Ds", WIDTH_DS)
def test_gpu_every_assignment_width(gpu, Ds):
    c, ref_cb, ref, ref_pot, seeded = width_case(Ds)
    cb, st = _gpu_train(gpu, c)
    assert_run_equals("Ds %d (width %d)" % (Ds, padded(Ds)), (cb, st), (ref_cb, ref))
    pot = gpu.train_potential(c["vectors"], cb)
    print("potential gpu", pot.tolist(), "restatement", ref_pot.tolist())
    assert np.array_equal(bits64(pot), bits64(ref_pot))
    if seeded is not None:
        assert_seeding_equals("Ds %d" % Ds, gpu.kmeanspp_seed(c["vectors"], M=c["M"], K=c["K"], seed=c["seed"]), seeded)


@pytest.mark.gpu
def test_gpu_past_the_first_upload_and_the_first_chunk_of_leaves(gpu):
    c, ref_cb, ref, ref_pot, seeded = past_case()
    cb, st = _gpu_train(gpu, c)
    assert_run_equals("past 2**18", (cb, st), (ref_cb, ref))
    print("distortion gpu", st["distortion"], "restatement", ref["distortion"])
    assert st["distortion"] == ref["distortion"]                           # integers: exact in any order
    assert np.array_equal(bits64(gpu.train_potential(c["vectors"], cb)), bits64(ref_pot))
    assert_seeding_equals("past 2**18", gpu.kmeanspp_seed(c["vectors"], M=c["M"], K=c["K"], seed=PAST_SEED), seeded)


@pytest.mark.gpu
def test_gpu_binades_potential_is_infinite_and_the_seedings(gpu):
    c, seeded, seed_pot, _ = seeding_case("binades")
    got = gpu.train_potential(c["vectors"], seeded)
    print("potential gpu", got.tolist(), "restatement", P.potential(c["vectors"], seeded).tolist())
    assert got[1] == np.inf
    assert np.array_equal(bits64(got), bits64(P.potential(c["vectors"], seeded)))
    assert np.array_equal(bits64(got), bits64(seed_pot))


@pytest.mark.gpu
def test_gpu_restarts_that_tie_at_infinity_keep_run_0(gpu):
    """A kernel that reports the FLT_MAX its search starts from keeps run 2 in sub-space 1 here, with a distortion of
    1.02e39 (seen on an MI355X before train_assign_kernel reported the computed distance)."""
    c, (ref_cb, ref) = restart_case()
    cb, st = gpu.train_codebook(**c)
    print("distortion gpu", st["distortion"], "restatement", ref["distortion"])
    for m in range(c["M"]):
        kept = [r for r, (run_cb, _, _) in enumerate(ref["runs"]) if np.array_equal(bits(cb[m]), bits(run_cb[m]))]
        print("sub-space", m, "gpu kept run", kept, "restatement", ref["winner"][m])
    assert np.array_equal(bits(cb), bits(ref_cb))
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (ref["iters_run"], ref["converged"], ref["reseeded"])
    assert st["distortion"][0] == np.inf
    assert np.array_equal(np.isinf(st["distortion"]), np.isinf(ref["distortion"]))
    single = dict(c, restarts=1)
    pot = gpu.train_potential(c["vectors"], gpu.train_codebook(**single)[0])
    assert np.array_equal(bits64(pot), bits64(ref["runs"][0][2])) and pot[1] == np.inf


@pytest.mark.gpu
def test_gpu_exactly_flt_max_keeps_the_encoders_label_and_reports_infinity(gpu):
    c = flt_max_case()
    ref_cb, ref = R.train(**c)
    cb, st = _gpu_train(gpu, c)
    assert_run_equals("FLT_MAX", (cb, st), (ref_cb, ref))
    assert st["distortion"] == [np.inf]
    assert gpu.encode_pq(c["vectors"], c["init"])[:, 0].tolist() == [0, 1, 1, 1, 1]
    pot = gpu.train_potential(c["vectors"], c["init"])
    assert np.array_equal(bits64(pot), bits64(P.potential(c["vectors"], c["init"]))) and pot[0] == np.inf


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORNERS))
def test_gpu_corner_matches_the_restatement_bit_for_bit(gpu, name):
    c, ref_cb, ref = corner(name)
    cb, st = _gpu_train(gpu, c)
    assert_run_equals(name, (cb, st), (ref_cb, ref))
    n, M = len(c["vectors"]), c["M"]
    assert len(st["distortion"]) == len(ref["distortion"])
    for r, (got, want) in enumerate(zip(st["distortion"], ref["distortion"])):
        print("round %d distortion gpu %.17g restatement %.17g" % (r + 1, got, want))
        if name in EXACT_TRACE:
            assert got == want, (r, got, want)
        else:                                        # the order of this sum is free: test_train_codebook's bound
            assert abs(got - want) <= n * M * 2.0 ** -52 * want, (r, got, want)
    pot = gpu.train_potential(c["vectors"], cb)
    assert np.array_equal(bits64(pot), bits64(P.potential(c["vectors"], ref_cb)))
    if name == "all_padding":
        assert not cb[5:].any()
