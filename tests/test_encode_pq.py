"""The PQ encoder at its edges: encode_pq_kernel (dpq_kernels.hip) through dpq_encode_pq, api.encode_pq and
`deltapq -task encode`, against oracle/pq_encode_oracle.py (PQTree::EncodePlain, pq_tree.cpp:215-237, restated).

One table of named cases serves both sides.  On the CPU the restatement is pinned by a hand-derived case and by a
plain double loop, and every case is shown to reach what its name claims (a tie, an overflow, a NaN in front of the
minimum, a padded sub-space); on the GPU the kernel has to give the restatement's codes exactly."""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import pq_encode_oracle as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
DPQ_ERR_HIP = -5
TILE = 1 << 20                       # dpq_encode_pq uploads and encodes this many vectors at a time


# ---- the cases both sides run ---------------------------------------------------------------------------------------

# (n, D, M, K, Ds): random normal data, so that a padded column differs from what a wrong read would find there
SHAPES = [(1, 8, 8, 256, 1),
          (255, 24, 8, 7, 3), (256, 24, 8, 7, 3), (257, 24, 8, 7, 3),   # one block less one, one block, one more
          (1000, 128, 8, 256, 16),
          (1000, 128, 16, 200, 8),
          (513, 100, 8, 256, 16),    # D < M * Ds: sub-space 6 partly, sub-space 7 wholly padding
          (513, 140, 8, 256, 16),    # D > M * Ds: the last 12 columns are ignored
          (300, 1, 8, 2, 1),         # seven sub-spaces of zeros
          (300, 64, 2, 256, 32),     # the largest Ds of the reference's configurations: 64 KB of LDS
          (300, 64, 1, 256, 64)]     # the largest shape that fits: 128 KB of the launcher's 160 KB
TOO_WIDE = (300, 96, 1, 256, 96)     # 96 KB of codewords + 96 KB of sub-vectors: refused
PAD_SHORT = "shape_513x100_M8K256Ds16"


def _shape_case(n, D, M, K, Ds, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, D)).astype(np.float32), rng.normal(size=(M, K, Ds)).astype(np.float32)


def _case_ties():            # integers in -2..2: many duplicate codewords and many equidistant ones; sums are exact
    rng = np.random.default_rng(101)
    return (rng.integers(-2, 3, size=(600, 8)).astype(np.float32),
            rng.integers(-2, 3, size=(2, 256, 4)).astype(np.float32))


def _case_ties_reversed():   # the same codewords in the opposite order: the first minimum is another index
    v, cb = _case_ties()
    return v, np.ascontiguousarray(cb[:, ::-1])


def _case_overflow():        # 3e19 squared is +inf in fp32
    rng = np.random.default_rng(102)
    v = rng.normal(size=(200, 6)).astype(np.float32)
    cb = rng.normal(size=(3, 6, 2)).astype(np.float32)
    cb[:, 0, :] = 3e19       # codeword 0 of every sub-space: the first FINITE codeword has to win
    v[::5, 1] = 3e19         # sub-space 0 of every fifth vector: every distance is +inf, the code is 0
    v[2::10, 1] = -3e19
    return v, cb


def _case_nan():
    rng = np.random.default_rng(103)
    v = rng.normal(size=(200, 6)).astype(np.float32)
    cb = rng.normal(size=(3, 6, 2)).astype(np.float32)
    cb[:, 3, 0] = np.nan     # codeword 3 of every sub-space: skipped, wherever the minimum is
    cb[2, :, 1] = np.nan     # sub-space 2: nothing but NaN, the code is 0
    v[7, 0] = np.nan         # and one vector that is NaN against every codeword of sub-space 0
    return v, cb


def _case_subnormal():
    """Coordinates around 2^-70: every square is a subnormal (2^-149 .. 2^-126), and so is every distance.  With
    denormals flushed anywhere in subtract, multiply or add the distances collapse to zero and every code to 0.  Some
    coordinates are subnormal themselves, some are -0.0."""
    rng = np.random.default_rng(104)

    def draw(shape):
        x = rng.integers(1 << 23, 1 << 24, size=shape) * 2.0 ** rng.integers(-97, -89, size=shape)
        return (x * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)

    v, cb = draw((256, 4)), draw((2, 8, 2))
    v[::7, 0] = np.float32(2.0 ** -130)
    v[3::7, 1] = np.float32(-0.0)
    cb[0, 1, 0] = np.float32(-0.0)
    cb[1, 2, 1] = np.float32(-(2.0 ** -140))
    return v, cb


def _case_adversarial():
    """Coordinates spread over 2^-20 .. 2^20 inside one sub-vector, and every codeword has a neighbour a few ulps away
    in every coordinate: the two nearest distances of a vector differ in their last bits, so the winner depends on
    every rounding of the in-order fp32 sum (a fused multiply-add, a reordered or a wider sum picks the other one)."""
    rng = np.random.default_rng(105)
    n, M, K, Ds = 300, 2, 32, 8
    v = (rng.normal(size=(n, M * Ds)) * 2.0 ** rng.uniform(-20, 20, size=(n, M * Ds))).astype(np.float32)
    half = (rng.normal(size=(M, K // 2, Ds)) * 2.0 ** rng.uniform(-20, 20, size=(M, K // 2, Ds))).astype(np.float32)
    near = (half.view(np.int32) + rng.integers(-3, 4, size=half.shape).astype(np.int32)).view(np.float32)
    cb = np.empty((M, K, Ds), dtype=np.float32)
    cb[:, 0::2], cb[:, 1::2] = half, near
    return v, cb


TILE_BLOCK = {TILE - 1: (1, 1), TILE: (2, 3), TILE + 1: (4, 0)}     # vector -> its codes, by construction


def _case_tile_boundary():
    """2^20 + 257 vectors: the second upload of dpq_encode_pq, 257 vectors at base = 2^20.  Codeword k of both
    sub-spaces is (10 k, 10 k); the three vectors around the boundary ARE codewords, each of another pair, so a base
    that is off by one shows as a shifted block."""
    rng = np.random.default_rng(106)
    cb = np.repeat(10.0 * np.arange(5, dtype=np.float32), 2).reshape(1, 5, 2).repeat(2, axis=0)
    v = (rng.normal(size=(TILE + 257, 4)) * 15.0 + 20.0).astype(np.float32)
    for i, (a, b) in TILE_BLOCK.items():
        v[i] = (10 * a, 10 * a, 10 * b, 10 * b)
    return v, np.ascontiguousarray(cb)


def _shape_name(s):
    return "shape_%dx%d_M%dK%dDs%d" % s


CASES = {_shape_name(s): functools.partial(_shape_case, *s, seed=10 + i) for i, s in enumerate(SHAPES)}
CASES.update({f.__name__[6:]: f for f in (_case_ties, _case_ties_reversed, _case_overflow, _case_nan, _case_subnormal,
                                          _case_adversarial, _case_tile_boundary)})
assert PAD_SHORT in CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """(vectors, codebook, the restatement's codes); computed once, never written to."""
    v, cb = CASES[name]()
    codes = E.encode_pq(v, cb)
    for a in (v, cb, codes):
        a.setflags(write=False)
    return v, cb, codes


def loop_encode(vectors, codebook):
    """PQTree::EncodePlain as a plain double loop over np.float32 scalars (every operation rounds to fp32)."""
    n, D = vectors.shape
    M, K, Ds = codebook.shape
    codes = np.zeros((n, M), dtype=np.uint8)
    zero = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in range(n):
            for m in range(M):
                best, best_k = E.FLT_MAX, 0
                for k in range(K):
                    dist = zero
                    for d in range(Ds):
                        col = m * Ds + d
                        diff = (vectors[i, col] if col < D else zero) - codebook[m, k, d]
                        dist = dist + diff * diff
                    assert type(dist) is np.float32
                    if dist < best:
                        best, best_k = dist, k
                codes[i, m] = best_k
    return codes


HAND_CB = [[[0, 0], [4, 0], [0, 4]],         # sub-space 0
           [[1, 1], [-1, -1], [1, -3]]]      # sub-space 1
HAND = [  # vector              squared distances, sub-space 0 | sub-space 1      codes
    ([3, 3, 0, 0], [1, 0]),    # 18, 10, 10: 1 and 2 tie, 1 wins        | 2, 2, 10: 0 and 1 tie, 0 wins
    ([0, 2, 0, -2], [0, 1]),   # 4, 20, 4: 0 and 2 tie, 0 wins          | 10, 2, 2: 1 and 2 tie, 1 wins
    ([4, 1, 1, -3], [1, 2]),   # 17, 1, 25                              | 16, 8, 0
    ([-1, 5, 2, 2], [2, 0]),   # 26, 50, 2                              | 2, 18, 26
]


def check_hand_case(encode):
    v = np.array([h[0] for h in HAND], dtype=np.float32)
    got = encode(v, np.array(HAND_CB, dtype=np.float32))
    assert got.dtype == np.uint8 and got.tolist() == [h[1] for h in HAND]


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------

def test_restatement_on_the_hand_derived_case():
    check_hand_case(E.encode_pq)
    check_hand_case(loop_encode)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_agrees_with_the_double_loop(name):
    """At most 64 vectors of every case, fewer where M * K * Ds is large (the loop costs a microsecond a step)."""
    v, cb, codes = case(name)
    M, K, Ds = cb.shape
    keep = min(64, len(v), max(3, 120000 // (M * K * Ds)))           # a fraction of a second per case
    rows = np.arange(keep)
    if name == "tile_boundary":
        rows = np.concatenate((rows, np.arange(TILE - 2, TILE + 3)))
    assert np.array_equal(loop_encode(v[rows], cb), codes[rows])
    assert np.array_equal(E.encode_pq(v[rows], cb), codes[rows])     # a vector's code does not depend on its neighbours


def test_restatement_pads_short_and_ignores_long_vectors():
    rng = np.random.default_rng(0)
    v, cb = rng.normal(size=(50, 10)).astype(np.float32), rng.normal(size=(4, 9, 3)).astype(np.float32)
    padded = np.zeros((50, 12), dtype=np.float32)
    padded[:, :10] = v
    want = E.encode_pq(padded, cb)
    assert np.array_equal(E.encode_pq(v, cb), want)                                    # D = 10 < M * Ds = 12
    assert np.array_equal(E.encode_pq(np.hstack([padded, v]), cb), want)               # D = 22 > 12
    assert np.array_equal(E.encode_pq(v[:, :1], cb)[:, 1:], E.encode_pq(np.zeros((50, 12)), cb)[:, 1:])


def _two_smallest(dist):
    part = np.sort(dist, axis=1)
    return part[:, 0], part[:, 1]


def test_every_case_reaches_what_its_name_claims():
    """Non-vacuity, from the restatement's own distance matrices."""
    for name in ("ties", "ties_reversed"):
        v, cb, codes = case(name)
        for m in range(cb.shape[0]):
            dist = E.sub_distances(v, cb, m)
            lo, second = _two_smallest(dist)
            tied = lo.view(np.uint32) == second.view(np.uint32)
            assert tied.sum() >= 1, (name, m)
            first = (dist == lo[:, None]).argmax(1)
            assert np.array_equal(codes[:, m], first)                  # the lowest index of the minimum, everywhere
            assert (codes[tied, m] != (dist.shape[1] - 1 - (dist[:, ::-1] == lo[:, None]).argmax(1))[tied]).any()
    a, b = case("ties")[2], case("ties_reversed")[2]
    assert not np.array_equal(255 - a, b)            # mirrored codebook, NOT mirrored codes: the first minimum moved

    v, cb, codes = case("overflow")
    mixed = whole = 0
    for m in range(cb.shape[0]):
        dist = E.sub_distances(v, cb, m)
        inf, fin = np.isinf(dist).any(1), np.isfinite(dist).any(1)
        mixed += int((inf & fin).sum())
        whole += int((~fin).sum())
        assert np.all(codes[inf & fin, m] >= 1) and np.all(codes[~fin, m] == 0)
        assert not np.isnan(dist).any()
    assert mixed >= 1 and whole >= 1

    v, cb, codes = case("nan")
    behind = 0
    for m in range(cb.shape[0]):
        dist = E.sub_distances(v, cb, m)
        nan = np.isnan(dist)
        assert nan[:, 3].all()
        some = ~nan.all(1)
        assert np.array_equal(codes[some, m], np.nanargmin(dist[some], axis=1)) and not (codes[some, m] == 3).any()
        assert np.all(codes[~some, m] == 0)
        behind += int((codes[some, m] > 3).sum())                      # a NaN sits in front of the true minimum
        if some.any():
            assert (dist[some].argmin(1) == 3).all()                   # ... where numpy's argmin takes the NaN
    assert behind >= 1 and np.all(codes[:, 2] == 0) and codes[7, 0] == 0

    v, cb, codes = case("subnormal")
    tiny = np.finfo(np.float32).tiny
    for m in range(cb.shape[0]):
        dist = E.sub_distances(v, cb, m)
        assert ((dist > 0) & (dist < tiny)).mean() > 0.9               # subnormal distances, not zeros
        assert len(np.unique(codes[:, m])) >= 4                        # flushed to zero they would all be code 0
    assert np.signbit(v).any() and (v == 0).any() and ((np.abs(v) < tiny) & (v != 0)).any()

    v, cb, codes = case(PAD_SHORT)
    M, K, Ds = cb.shape
    D = v.shape[1]
    assert D < M * Ds and (M - 1) * Ds >= D and (M - 2) * Ds < D < (M - 1) * Ds     # 7 wholly, 6 partly padding
    assert np.all(codes[:, M - 1] == (cb[M - 1].astype(np.float64) ** 2).sum(1).argmin())
    assert len(np.unique(codes[:, M - 2])) > 1
    v, cb, _ = case("shape_513x140_M8K256Ds16")
    assert v.shape[1] > cb.shape[0] * cb.shape[2]

    v, cb, codes = case("tile_boundary")
    assert len(v) == TILE + 257
    for i, want in TILE_BLOCK.items():
        assert tuple(codes[i]) == want
    assert len({tuple(codes[i]) for i in TILE_BLOCK}) == 3
    assert len(np.unique(codes[TILE:], axis=0)) > 5


def test_adversarial_case_tells_the_stated_arithmetic_from_any_other():
    """On the adversarial case an fp64 argmin, and a sum whose products are not rounded on their own (what a fused
    multiply-add computes, up to a double rounding), pick another codeword than the in-order fp32 sum at least once."""
    v, cb, codes = case("adversarial")
    M, K, Ds = cb.shape
    sub = v.reshape(len(v), M, 1, Ds)
    exact = ((sub.astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(-1).argmin(-1)
    assert (exact != codes).sum() >= 1
    fused = np.zeros((len(v), M, K), dtype=np.float32)
    for d in range(Ds):
        diff = (sub[..., d] - cb[None, ..., d]).astype(np.float32).astype(np.float64)
        fused = (fused.astype(np.float64) + diff * diff).astype(np.float32)
    assert (fused.argmin(-1) != codes).sum() >= 1
    span = np.log2(np.abs(v).max(1) / np.abs(v).min(1))
    assert np.median(span) > 20


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
def test_gpu_hand_derived_case(gpu):
    check_hand_case(gpu.encode_pq)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "tile_boundary"))
def test_gpu_matches_the_restatement(gpu, name):
    v, cb, want = case(name)
    got = gpu.encode_pq(v, cb)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d of %d codes differ, first at (vector, sub-space) %s: kernel %d, restatement %d" % (
        len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_exact_ties_take_the_lowest_index(gpu):
    v, cb, want = case("ties")
    _, cb_rev, want_rev = case("ties_reversed")
    got, got_rev = gpu.encode_pq(v, cb), gpu.encode_pq(v, cb_rev)
    for m in range(cb.shape[0]):
        dist = E.sub_distances(v, cb, m)
        assert np.array_equal(got[:, m], (dist == dist.min(1)[:, None]).argmax(1))
    assert np.array_equal(got, want)
    assert np.array_equal(got_rev, want_rev)         # against the restatement, not by arithmetic on `got`


@pytest.mark.gpu
def test_gpu_non_finite_distances(gpu):
    v, cb, want = case("overflow")
    got = gpu.encode_pq(v, cb)
    assert np.array_equal(got, want)
    assert np.all(got[::5, 0] == 0) and np.all(got[1::5, 0] >= 1) and np.all(got[:, 1:] >= 1)
    v, cb, want = case("nan")
    got = gpu.encode_pq(v, cb)
    assert np.array_equal(got, want)
    assert np.all(got[:, 2] == 0) and got[7, 0] == 0 and not (got[:, :2] == 3).any()
    lone = np.full((1, 1, 2), np.nan, dtype=np.float32)              # the NaN codeword is the only one: code 0
    assert np.array_equal(gpu.encode_pq(v[:5, :2], lone), np.zeros((5, 1), dtype=np.uint8))
    assert np.array_equal(E.encode_pq(v[:5, :2], lone), np.zeros((5, 1), dtype=np.uint8))


@pytest.mark.gpu
def test_gpu_second_upload_tile(gpu):
    """n = 2^20 + 257: the 257 vectors of the second tile and the 2^20 before them, each compared on its own."""
    v, cb, want = case("tile_boundary")
    got = gpu.encode_pq(v, cb)
    assert got.shape == want.shape
    for i, codes in TILE_BLOCK.items():
        assert tuple(got[i]) == codes, (i, got[i - 2:i + 3].tolist())
    assert np.array_equal(got[TILE:], want[TILE:])
    assert np.array_equal(got[:TILE], want[:TILE])


@pytest.mark.gpu
def test_gpu_refuses_more_lds_than_the_launcher_allows(gpu):
    from deltapq_amd import _lib
    v, cb = _shape_case(*TOO_WIDE, seed=9)
    M, K, Ds = cb.shape
    assert (K * Ds + Ds * 256) * 4 > 160 * 1024
    with pytest.raises(_lib.DpqError) as e:
        gpu.encode_pq(v, cb)
    assert e.value.status == DPQ_ERR_HIP
    v, cb, want = case("shape_300x64_M1K256Ds64")                    # a valid call still works afterwards
    assert np.array_equal(gpu.encode_pq(v, cb), want)


@pytest.mark.gpu
def test_gpu_no_vectors(gpu):
    _, cb, _ = case("shape_255x24_M8K7Ds3")
    got = gpu.encode_pq(np.zeros((0, 24), dtype=np.float32), cb)
    assert got.shape == (0, 8) and got.dtype == np.uint8


@pytest.mark.gpu
def test_gpu_cli_encodes_short_vectors(gpu, tmp_path):
    """`-task encode` with D = 100 under an M8K256 codebook of Ds = 16: the CLI takes Ds from the codewords file and
    does not ask for D == M * Ds (dpq_cli.cpp, task "encode"), so the zero-padded path runs through it."""
    from deltapq_amd import synth
    d = str(tmp_path)
    rng = np.random.default_rng(7)
    base = rng.normal(size=(700, 100)).astype(np.float32)
    cb = rng.normal(size=(8, 256, 16)).astype(np.float32)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    gpu.write_codewords(os.path.join(d, "M8K256codewords.txt"), cb)
    assert np.array_equal(gpu.read_codewords(os.path.join(d, "M8K256codewords.txt")).view(np.uint32), cb.view(np.uint32))
    r = subprocess.run([EXE, "-dataset", d, "-task", "encode", "-m", "8", "-k", "256"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = os.path.join(d, "want.plain")
    gpu.write_codes_plain(want, E.encode_pq(base, cb))
    with open(os.path.join(d, "codes.bin.plain.M8K256N700"), "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
