"""The k-means++ start and the restarts of dpq_train_codebook, dpq_kmeanspp_seed, dpq_train_potential,
`deltapq -task learn -init pp -restarts R`.

The rules are this build's own (include/deltapq_amd.h), restated on the CPU in
tests/_kmeanspp_restatement.py; the GPU has to meet that restatement bit for bit, with no tolerance anywhere."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import _kmeans_restatement as R
import _kmeanspp_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")
ERR_ARG, ERR_NO_DEVICE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the seeding cases both sides run --------------------------------------------------------------------------------

def _real(n, D, seed):
    return np.random.default_rng(seed).normal(size=(n, D)).astype(np.float32)


def _case_basic():            # Ds = 5, padded to the kernel's width; four leaves, the last one short
    return dict(vectors=_real(1000, 18, 1), M=4, K=16, seed=3)


def _case_short_leaf():       # a single short leaf
    return dict(vectors=_real(200, 8, 2), M=2, K=2, seed=1)


def _case_leaf_of_one():      # a second leaf holding one vector
    return dict(vectors=_real(257, 8, 3), M=2, K=4, seed=7)


def _case_many_leaves():      # 274 leaves: the T chain and the leaf search cross many blocks
    return dict(vectors=_real(70000, 8, 4), M=2, K=32, seed=11)


def _case_duplicates():       # 10 distinct rows, K = 16: the total reaches zero after at most 10 centres
    return dict(vectors=np.tile(_real(10, 8, 5), (60, 1)), M=2, K=16, seed=2)


BINADES_SEED = 0x8F2A5C93E4D17B06


def _case_binades():
    """Rows scaled by 2**+-20: the weights span 80 binades, far more than an fp64 sum holds, so only the stated order
    of the adds gives the stated bits.  Sub-space 0 is just that.  In sub-space 1 three rows are scaled further, to
    about 2**65, so that their fp32 distances overflow to +inf: that is what takes the fallbacks.  With finite weights
    r = u * total stays below the total (u <= 1 - 2**-53) and r' reaches a leaf's own sum only when r sits within an
    ulp or two of a running total, so no seed one can search for gets there.  A total of +inf does at once: no T_l
    exceeds r = +inf (the last leaf with S_l > 0 is taken), and no running sum exceeds r' (the leaf's last row with
    w_i > 0 is taken).  test_binades_case_takes_the_fallbacks checks that on the CPU."""
    rng = np.random.default_rng(6)
    n = 1500
    v = rng.normal(size=(n, 8)) * 2.0 ** rng.choice([-20.0, 20.0], size=(n, 1))
    v = v.astype(np.float32)
    v[[40, 700, 1301], 4:] *= np.float32(2.0 ** 45)     # a squared difference of these is beyond fp32
    return dict(vectors=v, M=2, K=12, seed=BINADES_SEED)


CASES = {f.__name__[6:]: f for f in (_case_basic, _case_short_leaf, _case_leaf_of_one, _case_many_leaves, _case_duplicates,
                                      _case_binades)}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    with np.errstate(all="ignore"):
        cb, pot, info = P.kmeanspp_seed(c["vectors"], c["M"], c["K"], c["seed"])
    return c, cb, pot, info


TRAIN = dict(M=4, K=16, max_iters=6, seed=21)


@functools.lru_cache(maxsize=None)
def train_vectors():
    from deltapq_amd import synth
    return synth.make_clustered_vectors(3000, 18, seed=12, n_clusters=40, spread=9.0) + _real(3000, 18, 13) * np.float32(0.25)


# ---- CPU -------------------------------------------------------------------------------------------------------------

def _train_raw(lib, v, M, K, **opts):
    from deltapq_amd import _lib
    n, D = v.shape
    cb = np.zeros((M, K, -(-D // M)), dtype=np.float32)
    o = _lib.TrainOpts(device=0, max_iters=5, seed=0, **opts)
    return lib.dpq_train_codebook(ctypes.c_void_p(v.ctypes.data), n, D, M, K, o, ctypes.c_void_p(cb.ctypes.data), None)


def test_new_argument_errors_come_before_any_device_call(lib):
    v = np.zeros((300, 16), dtype=np.float32)
    assert _train_raw(lib, v, 2, 16, init=2) == ERR_ARG
    assert b"init" in lib.dpq_last_error()
    assert _train_raw(lib, v, 2, 16, init=-1) == ERR_ARG
    assert _train_raw(lib, v, 2, 16, restarts=17) == ERR_ARG
    assert b"restarts" in lib.dpq_last_error()
    assert _train_raw(lib, v, 2, 16, restarts=-1) == ERR_ARG
    assert _train_raw(lib, v, 2, 16, init=1, use_initial=1) == ERR_ARG
    assert b"use_initial" in lib.dpq_last_error()


def _seed_raw(lib, v, M, K, out="alloc"):
    n, D = v.shape
    cb = np.zeros((max(M, 1), max(K, 1), -(-D // max(M, 1))), dtype=np.float32)
    return lib.dpq_kmeanspp_seed(ctypes.c_void_p(v.ctypes.data), n, D, M, K, 0, 0,
                                 ctypes.c_void_p(cb.ctypes.data) if out == "alloc" else None, None)


def _potential_raw(lib, v, M, K, Ds=None, out="alloc"):
    n, D = v.shape
    Ds = Ds or -(-D // max(M, 1))
    cb = np.zeros((max(M, 1), max(K, 1), Ds), dtype=np.float32)
    pot = np.zeros(max(M, 1), dtype=np.float64)
    return lib.dpq_train_potential(ctypes.c_void_p(v.ctypes.data), n, D, ctypes.c_void_p(cb.ctypes.data), M, K, Ds, 0,
                                   ctypes.c_void_p(pot.ctypes.data) if out == "alloc" else None)


def test_argument_errors_of_the_new_functions(lib):
    v = np.zeros((300, 16), dtype=np.float32)
    for raw in (_seed_raw, _potential_raw):
        assert raw(lib, v, 2, 16, out=None) == ERR_ARG
        assert raw(lib, v, 2, 1) == ERR_ARG           # K outside 2..256
        assert raw(lib, v, 2, 257) == ERR_ARG
        assert raw(lib, v[:15], 2, 16) == ERR_ARG     # K > n
        assert raw(lib, v, 0, 16) == ERR_ARG          # M < 1
        assert raw(lib, np.zeros((300, 160), dtype=np.float32), 1, 256) == ERR_ARG
        assert b"LDS" in lib.dpq_last_error()
    assert _potential_raw(lib, v, 2, 16, Ds=7) == ERR_ARG   # Ds is ceil(D / M)


def test_new_calls_without_gpu_fail_loudly(lib):
    from deltapq_amd import api
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    v = np.zeros((300, 16), dtype=np.float32)
    assert _train_raw(lib, v, 2, 16, init=1, restarts=16) == ERR_NO_DEVICE
    with pytest.raises(api.DpqError) as e:
        api.kmeanspp_seed(v, M=2, K=16)
    assert e.value.status == ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(api.DpqError) as e:
        api.train_potential(v, np.zeros((2, 16, 8), dtype=np.float32))
    assert e.value.status == ERR_NO_DEVICE


def test_new_symbols_declared_exported_and_bound(lib):
    from deltapq_amd import _lib, api
    names = {name for name, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "deltapq_amd.h")).read()
    for name in ("dpq_kmeanspp_seed", "dpq_train_potential"):
        assert name in names
        assert name + "(" in header
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert ctypes.sizeof(_lib.TrainOpts) == 4 + 4 + 8 + 4 + 3 * 4      # the struct did not grow
    assert _lib.TrainOpts.init.offset == 20 and _lib.TrainOpts.restarts.offset == 24
    assert callable(api.kmeanspp_seed) and callable(api.train_potential)
    with pytest.raises(ValueError):
        api.train_codebook(np.zeros((300, 16), dtype=np.float32), M=2, K=16, start="pp")


def test_restatement_on_the_hand_derived_case():
    """M = 1, Ds = 1, n = 8, K = 3, seed 0, one leaf.  splitmix64 from state 0 gives the published outputs
        z0 = 0xE220A8397B1DCDAF, z1 = 0x6E789E6AA1B965F4, z2 = 0x06C45D188009454F.
    Centre 0 is row z0 % 8 = 0xF % 8 = 7.  u1 = (z1 >> 11) * 2**-53 = 0.43152799704850997 (z1 / 2**64 = 0x6E78.. / 2**64,
    0x6E / 0x100 = 0.4297 and a little), u2 = 0.026433771592597743 (0x06C4 / 0x10000 = 0.02643).

    x = 0 1 2 3 4 6 8 5: centre 0 is x7 = 5, w = 25 16 9 4 1 1 9 0, S_0 = total = 65, all exact.
      step 1  r = u1 * 65 = 28.05; the running sums 25, 41: 41 > 28.05 first at row 1.  Centre 1 = x1 = 1.
              w = min(w, (x - 1)**2) = 1 0 1 4 1 1 9 0, total 17.
      step 2  r = u2 * 17 = 0.449; the running sum 1 > 0.449 at row 0.  Centre 2 = x0 = 0.
              w = min(w, x**2) = 0 0 1 4 1 1 9 0: the potential is 16.
    x = 2 2 2 2 7 7 7 7 (two distinct values, K = 3): centre 0 is x7 = 7, w = 25 25 25 25 0 0 0 0, total 100.
      step 1  r = u1 * 100 = 43.15; the running sums 25, 50: row 1.  w = 0 everywhere.
      step 2  total == 0: the smallest index that is no centre yet; 7 and 1 are, so row 0.  Potential 0."""
    g = P.Rng(0)
    assert [g.next() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert P.Rng(5, 2).s == (5 + 2 * 0xD6E8FEB86659FD93) % 2 ** 64
    x = np.array([[0], [1], [2], [3], [4], [6], [8], [5]], dtype=np.float32)
    rows, w, pot, how = P.seed_subspace(x, 3, 0)
    assert rows == [7, 1, 0] and how == ["walk", "walk"]
    assert w.tolist() == [0, 0, 1, 4, 1, 1, 9, 0] and pot == 16.0
    assert P.distance_to(x, 7).tolist() == [25, 16, 9, 4, 1, 1, 9, 0]
    i, _ = P.draw(np.array([25, 16, 9, 4, 1, 1, 9, 0], dtype=np.float32), 0x6E789E6AA1B965F4, [7])
    assert i == 1 and 25 < 0.43152799704850997 * 65 < 41
    cb, pots, _ = P.kmeanspp_seed(x, 1, 3, 0)
    assert cb.tolist() == [[[5.0], [1.0], [0.0]]] and pots.tolist() == [16.0]
    assert P.potential(x, cb).tolist() == [16.0]        # the seeding's final weights are one assignment's distances

    d = np.array([[2], [2], [2], [2], [7], [7], [7], [7]], dtype=np.float32)
    rows, w, pot, how = P.seed_subspace(d, 3, 0)
    assert rows == [7, 1, 0] and how == ["walk", "zero"]
    assert not w.any() and pot == 0.0


def test_restatement_leaf_rule_and_fallbacks():
    """The leaf rule on weights made by hand, two leaves each."""
    import math
    # 1.0 and then 2**-60, 257 times: every later add of leaf 0 is absorbed (half an ulp of 1.0 is 2**-53), so
    # S_0 = 1, S_1 = 2**-59, T_1 = 1 + 2**-59 = 1: the order of the adds is the contract, the exact sum is not.
    w = np.full(258, 2.0 ** -60, dtype=np.float32)
    w[0] = 1.0
    S, T = P.leaf_totals(w)
    assert S.tolist() == [1.0, 2.0 ** -59] and T.tolist() == [1.0, 1.0]
    assert math.fsum(w.astype(np.float64)) == 1.0 + 257 * 2.0 ** -60
    z_half, z_top = 1 << 63, (1 << 64) - 1                     # u = 0.5 and u = 1 - 2**-53
    assert P.draw(w, z_half, [5]) == (0, "walk")
    assert P.draw(w, z_top, [5]) == (0, "walk")                # r = 1 - 2**-53 < T_0 = 1
    # 256 ones and a three: S = 256, 3, T = 256, 259.  u = 0.5: r = 129.5, leaf 0, the running sum i + 1 passes it
    # at row 129.  u = 1 - 2**-53: r just below 259, leaf 1, r' just below 3, the running sum 3 passes it at row 256.
    w = np.ones(257, dtype=np.float32)
    w[256] = 3.0
    assert P.leaf_totals(w)[1].tolist() == [256.0, 259.0]
    assert P.draw(w, z_half, [0]) == (129, "walk")
    assert P.draw(w, z_top, [0]) == (256, "walk")
    # total = +inf: nothing exceeds r, both fallbacks; leaf 1 is the last with S_l > 0, row 257 its last with w_i > 0
    inf = np.full(258, 2.0 ** -60, dtype=np.float32)
    inf[3] = np.inf
    with np.errstate(all="ignore"):
        assert P.draw(inf, z_half, [3]) == (257, "leaf-fallback+row-fallback")
    assert P.draw(np.zeros(300, dtype=np.float32), z_half, [0, 1, 3]) == (2, "zero")


def test_binades_case_takes_the_fallbacks():
    """The check the GPU case relies on: steps of the binades input take the fallbacks (sub-space 1), and sub-space 0
    draws by ordinary walks over weights of many binades."""
    c, _, pot, info = case("binades")
    for m in range(c["M"]):
        print("sub-space", m, info["how"][m], "potential", pot[m])
    assert all(h == "walk" for h in info["how"][0]) and np.isfinite(pot[0])
    sub0 = R.split(c["vectors"], 2)[0]
    w = P.distance_to(sub0, info["rows"][0][0])
    assert np.log2(w[w > 0].max() / w[w > 0].min()) > 60          # more binades than an fp64 sum holds
    assert any("leaf-fallback" in h for h in info["how"][1]) and any("row-fallback" in h for h in info["how"][1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_seeding_is_a_valid_start(name):
    c, cb, pot, info = case(name)
    n = len(c["vectors"])
    for m, sub in enumerate(R.split(c["vectors"], c["M"])):
        rows = info["rows"][m]
        assert len(rows) == c["K"] and all(0 <= r < n for r in rows)
        assert len(set(rows)) == c["K"]                        # a row with w_i == 0 is never drawn again
        assert np.array_equal(bits(cb[m]), bits(sub[rows]))
    if name == "duplicates":
        assert all("zero" in h for h in info["how"]) and not pot.any()
    if name == "many_leaves":
        assert max(max(r) for r in info["rows"]) >= 256 * 100   # centres come from far leaves too


def test_restatement_restart_rule():
    v = train_vectors()[:600]
    cb, st = P.train(v, 2, 8, max_iters=4, seed=5, restarts=3)
    singles = [R.train(v, 2, 8, 4, 5 + r) for r in range(3)]
    pots = np.stack([P.potential(v, s[0]) for s in singles])
    for m in range(2):
        assert np.array_equal(bits(cb[m]), bits(singles[int(pots[:, m].argmin())][0][m]))
    assert st["reseeded"] == sum(s[1]["reseeded"] for s in singles)
    assert st["distortion"] == singles[0][1]["distortion"]


# ---- GPU -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


@pytest.mark.gpu
def test_gpu_hand_derived_case(gpu):
    x = np.array([[0], [1], [2], [3], [4], [6], [8], [5]], dtype=np.float32)
    cb, pot = gpu.kmeanspp_seed(x, M=1, K=3, seed=0)
    assert cb.tolist() == [[[5.0], [1.0], [0.0]]] and pot.tolist() == [16.0]
    d = np.array([[2], [2], [2], [2], [7], [7], [7], [7]], dtype=np.float32)
    cb, pot = gpu.kmeanspp_seed(d, M=1, K=3, seed=0)
    assert cb.tolist() == [[[7.0], [2.0], [2.0]]] and pot.tolist() == [0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_seeding_matches_the_restatement_bit_for_bit(gpu, name):
    c, ref_cb, ref_pot, info = case(name)
    cb, pot = gpu.kmeanspp_seed(c["vectors"], M=c["M"], K=c["K"], seed=c["seed"])
    for m, sub in enumerate(R.split(c["vectors"], c["M"])):
        wrong = [j for j in range(c["K"]) if not np.array_equal(bits(cb[m, j]), bits(ref_cb[m, j]))]
        print(name, "sub-space", m, "potential gpu %r restatement %r" % (pot[m], ref_pot[m]), "first differing centre",
              wrong[:1])
        assert not wrong, "sub-space %d: centres %s differ from the restatement" % (m, wrong)
    assert np.array_equal(bits64(pot), bits64(ref_pot))
    again, pot2 = gpu.kmeanspp_seed(c["vectors"], M=c["M"], K=c["K"], seed=c["seed"])
    assert again.tobytes() == cb.tobytes() and pot2.tobytes() == pot.tobytes()


@pytest.mark.gpu
def test_gpu_duplicates_zero_total_then_the_trainers_repair(gpu):
    """16 centres from 10 distinct rows: six duplicate centres, so the first round leaves empty clusters to repair."""
    c, ref_seed, _, _ = case("duplicates")
    cb, st = gpu.train_codebook(c["vectors"], M=c["M"], K=c["K"], max_iters=4, seed=c["seed"], start="kmeans++")
    ref_cb, ref = R.train(c["vectors"], c["M"], c["K"], 4, 0, ref_seed)
    assert ref["reseeded"] >= 6
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (ref["iters_run"], ref["converged"], ref["reseeded"])
    assert np.array_equal(bits(cb), bits(ref_cb))


@pytest.mark.gpu
def test_gpu_start_kmeanspp_equals_use_initial_on_the_seeding(gpu):
    v = train_vectors()
    seeded, _ = gpu.kmeanspp_seed(v, M=TRAIN["M"], K=TRAIN["K"], seed=TRAIN["seed"])
    a, sa = gpu.train_codebook(v, start="kmeans++", **TRAIN)
    b, sb = gpu.train_codebook(v, init=seeded, **TRAIN)
    assert a.tobytes() == b.tobytes()
    assert sa["distortion"] == sb["distortion"] and sa["iters_run"] == sb["iters_run"]
    ref_cb, ref = P.train(v, start="kmeans++", **TRAIN)
    assert np.array_equal(bits(a), bits(ref_cb)) and sa["reseeded"] == ref["reseeded"]


@pytest.mark.gpu
def test_gpu_rows_start_with_one_run_is_unchanged(gpu):
    v = train_vectors()
    ref_cb, ref = R.train(v, TRAIN["M"], TRAIN["K"], TRAIN["max_iters"], TRAIN["seed"])   # pins the bytes of the rows start
    for kw in ({}, dict(start="rows", restarts=1), dict(restarts=0)):
        cb, st = gpu.train_codebook(v, **TRAIN, **kw)
        assert np.array_equal(bits(cb), bits(ref_cb)), kw
        assert (st["iters_run"], st["converged"], st["reseeded"]) == (ref["iters_run"], ref["converged"], ref["reseeded"])


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["rows", "kmeans++"])
def test_gpu_restarts_keep_the_lowest_potential_per_subspace(gpu, start):
    v = train_vectors()
    M = TRAIN["M"]
    cb, st = gpu.train_codebook(v, start=start, restarts=3, **TRAIN)
    kw = dict(TRAIN)
    singles = []
    for r in range(3):
        kw["seed"] = TRAIN["seed"] + r
        singles.append(gpu.train_codebook(v, start=start, **kw))
    pots = np.stack([gpu.train_potential(v, s[0]) for s in singles])       # [run][M]
    winner = pots.argmin(0)                                                # the first minimum: ties to the lowest r
    print(start, "potentials", pots.tolist(), "winner", winner.tolist())
    for m in range(M):
        assert np.array_equal(bits(cb[m]), bits(singles[winner[m]][0][m])), m
    assert st["reseeded"] == sum(s[1]["reseeded"] for s in singles)
    assert st["iters_run"] == max(s[1]["iters_run"] for s in singles)
    assert st["converged"] == int(all(s[1]["converged"] for s in singles))
    run0 = singles[0][1]["distortion"]
    assert st["distortion"][:len(run0)] == run0 and not any(st["distortion"][len(run0):])
    assert st["gpu_ms"] > 0 and st["assign_ms"] > 0 and st["wall_ms"] > 0
    ref_cb, ref = P.train(v, start=start, restarts=3, **TRAIN)
    assert ref["winner"] == winner.tolist()
    assert np.array_equal(bits(cb), bits(ref_cb))


@pytest.mark.gpu
def test_gpu_potential_matches_the_restatement(gpu):
    from deltapq_amd import synth
    c, seeded, seed_pot, _ = case("many_leaves")
    got = gpu.train_potential(c["vectors"], seeded)
    assert np.array_equal(bits64(got), bits64(P.potential(c["vectors"], seeded)))
    assert np.array_equal(bits64(got), bits64(seed_pot))                   # the seeding's weights are those distances
    v = train_vectors()
    cb = synth.make_codebook(3, 16, 6, seed=4)                             # any codebook, Ds = 6 padded
    assert np.array_equal(bits64(gpu.train_potential(v, cb)), bits64(P.potential(v, cb)))


@pytest.mark.gpu
def test_gpu_cli_learn_with_kmeanspp_and_restarts(gpu, tmp_path):
    from deltapq_amd import synth
    d = str(tmp_path)
    v = train_vectors()[:1500]
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), v)
    r = subprocess.run([EXE, "-dataset", d, "-task", "learn", "-m", "3", "-k", "16", "-init", "pp", "-restarts", "2",
                        "-seed", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cb = gpu.read_codewords(os.path.join(d, "M3K16codewords.txt"))
    want, _ = gpu.train_codebook(v, M=3, K=16, seed=5, start="kmeans++", restarts=2)
    assert np.array_equal(bits(cb), bits(want))
    rows, _ = gpu.train_codebook(v, M=3, K=16, seed=5)
    assert not np.array_equal(bits(rows), bits(want))
    r = subprocess.run([EXE, "-dataset", d, "-task", "learn", "-m", "3", "-k", "16", "-init", "random"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "-init rows|pp" in r.stdout
