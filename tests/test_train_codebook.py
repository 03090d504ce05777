"""Codebook learning on the GPU: dpq_train_codebook, dpq_write_codewords, `deltapq -task learn`.

No reference semantics (cv::kmeans): the rules are this build's own (include/deltapq_amd.h),
restated on the CPU in tests/_kmeans_restatement.py; the GPU has to meet that restatement bit for bit."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import _kmeans_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")


# ---- the cases both sides run ---------------------------------------------------------------------------------------

def _clustered(n, D, seed, n_clusters=300, spread=9.0):
    from deltapq_amd import synth
    return synth.make_clustered_vectors(n, D, seed=seed, n_clusters=n_clusters, spread=spread)


def _case_a_seed():      # (a) integer-valued: sums exact in any order, isolates the assignment and the rules
    return dict(vectors=_clustered(20000, 128, 1), M=8, K=256, max_iters=5, seed=3, init=None)


def _case_a_init():      # (a) from a given initial codebook
    from deltapq_amd import synth
    return dict(vectors=_clustered(20000, 32, 2, 200), M=2, K=64, max_iters=8, seed=0,
                init=synth.make_codebook(2, 64, 16, seed=5))


def _case_b_real():      # (b) wide exponent spread: only the stated summation order gives the stated bits
    rng = np.random.default_rng(21)
    v = rng.normal(size=(20000, 32)) * 10.0 ** rng.uniform(-3, 3, size=(20000, 32))
    return dict(vectors=v.astype(np.float32), M=2, K=64, max_iters=8, seed=11, init=None)


def _case_c_m16():       # (c) M = 16
    return dict(vectors=_clustered(20000, 128, 4), M=16, K=64, max_iters=5, seed=1, init=None)


def _case_d_ragged():    # (d) D not a multiple of M: Ds = 13, the last sub-space zero padded
    return dict(vectors=_clustered(20000, 100, 5), M=8, K=32, max_iters=5, seed=2, init=None)


def _case_d_wide():      # (d) Ds = 50: the one-vector-per-thread width of the assignment kernel
    return dict(vectors=_clustered(5000, 100, 6), M=2, K=16, max_iters=4, seed=2, init=None)


def _case_e_tiny():      # (e) K = 16, n barely above K
    rng = np.random.default_rng(9)
    return dict(vectors=rng.integers(0, 50, size=(20, 8)).astype(np.float32), M=2, K=16, max_iters=25, seed=9, init=None)


def _case_f_dups():      # (f) a start with many duplicate rows: 47 empty clusters per sub-space in round one
    v = _clustered(20000, 32, 7)
    rows = [0] * 48 + list(range(1, 17))
    return dict(vectors=v, M=2, K=64, max_iters=8, seed=0, init=np.stack([s[rows] for s in R.split(v, 2)]))


def _case_g_stop():      # run until the stop rule ends it: the monotonicity bound matters close to convergence
    return dict(vectors=_clustered(2000, 8, 8, 20, 3.0), M=2, K=8, max_iters=64, seed=4, init=None)


CASES = {f.__name__[6:]: f for f in (_case_a_seed, _case_a_init, _case_b_real, _case_c_m16, _case_d_ragged, _case_d_wide,
                                      _case_e_tiny, _case_f_dups, _case_g_stop)}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    cb, st = R.train(c["vectors"], c["M"], c["K"], c["max_iters"], c["seed"], c["init"])
    return c, cb, st


def assert_monotone(distortion, Ds):
    """Lloyd is monotone in exact arithmetic; each fp32 winning distance is within about (Ds + 2) * 2**-24 relative
    of its exact value, so a round may exceed the one before by at most a relative 4 * (Ds + 2) * 2**-24."""
    bound = 4 * (Ds + 2) * 2.0 ** -24
    for r in range(1, len(distortion)):
        print("round %d: %.17g -> %.17g" % (r, distortion[r - 1], distortion[r]))
        assert distortion[r] <= distortion[r - 1] * (1 + bound), (r, distortion[r - 1], distortion[r])


# ---- CPU ------------------------------------------------------------------------------------------------------------

def _train_raw(lib, v, M, K, max_iters=5, codewords="alloc", vectors="given"):
    from deltapq_amd import _lib
    n, D = v.shape
    cb = np.zeros((max(M, 1), max(K, 1), -(-D // max(M, 1))), dtype=np.float32)
    opts = _lib.TrainOpts(device=0, max_iters=max_iters, seed=0, use_initial=0)
    return lib.dpq_train_codebook(ctypes.c_void_p(v.ctypes.data) if vectors == "given" else None, n, D, M, K, opts,
                                  ctypes.c_void_p(cb.ctypes.data) if codewords == "alloc" else None, None)


def test_argument_errors_come_before_any_device_call(lib):
    v = np.zeros((300, 16), dtype=np.float32)
    assert _train_raw(lib, v, 2, 16, vectors=None) == -1
    assert _train_raw(lib, v, 2, 16, codewords=None) == -1
    assert _train_raw(lib, v, 2, 1) == -1            # K outside 2..256
    assert _train_raw(lib, v, 2, 257) == -1
    assert _train_raw(lib, v[:15], 2, 16) == -1      # K > n
    assert _train_raw(lib, v, 0, 16) == -1           # M < 1
    assert _train_raw(lib, v, 2, 16, max_iters=0) == -1
    assert _train_raw(lib, v, 2, 16, max_iters=65) == -1
    assert _train_raw(lib, np.zeros((300, 4096), dtype=np.float32), 1, 256) == -1   # 4 MB of codewords per sub-space
    assert _train_raw(lib, np.zeros((300, 160), dtype=np.float32), 1, 256) == -1    # 160 KB of codewords + the histogram
    assert b"LDS" in lib.dpq_last_error()


def test_train_without_gpu_fails_loudly(lib):
    from deltapq_amd import api
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.DpqError) as e:
        api.train_codebook(np.zeros((300, 16), dtype=np.float32), M=2, K=16)
    assert e.value.status == -4 and "no CPU fallback" in str(e.value)


def test_write_codewords_reads_back_the_same_bits(lib, tmp_path):
    from deltapq_amd import api, synth
    rng = np.random.default_rng(3)
    cb = (rng.normal(size=(3, 5, 4)) * 10.0 ** rng.uniform(-6, 6, size=(3, 5, 4))).astype(np.float32)
    cb[0, 0] = [1.0 / 3.0, 1e-7, 218.25, -0.1]
    cb[1, 1] = [-1.0 / 3.0, 16777217.0, 0.0, 3.4e38]
    path = str(tmp_path / "M3K5codewords.txt")
    api.write_codewords(path, cb)
    assert np.array_equal(api.read_codewords(path).view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(synth.read_codewords_txt(path).view(np.uint32), cb.view(np.uint32))
    # the reference's own six digits do lose bits, which is why dpq_write_codewords writes nine
    synth.write_codewords_txt(path, cb)
    assert not np.array_equal(api.read_codewords(path).view(np.uint32), cb.view(np.uint32))


HAND_POINTS = np.array([[0.0], [10.0], [2.5], [7.5], [5.0], [5.0]], dtype=np.float32)
HAND_INIT = np.array([[[5.0], [1000.0]]], dtype=np.float32)
HAND_CODEBOOK = np.array([[[6.875], [1.25]]], dtype=np.float32)
HAND_DISTORTION = [62.5, 37.5, 26.5, 20.3125]


def check_hand_case(train):
    """Ds = 1, K = 2, six points x = 0, 10, 2.5, 7.5, 5, 5 (vector index 0..5), start c = (5, 1000).  Every number
    below is exact in fp32.

    round 1  distances to c0 = 5: 25, 25, 6.25, 6.25, 0, 0, all far below those to 1000: labels 0 0 0 0 0 0,
             distortion 62.5, cluster 1 empty.  Update c0 = 30 / 6 = 5.  Repair: the largest winning distance, 25,
             is shared by vectors 0 and 1; the lower index donates: c1 = x0 = 0.           (the repair rule decides)
    round 2  c = (5, 0).  x = 2.5 is 6.25 from both codewords: the lower k wins, label 0.       (the tie rule decides)
             labels 1 0 0 0 0 0, one change, distortion 0 + 25 + 6.25 + 6.25 + 0 + 0 = 37.5.
             Update c0 = (10 + 2.5 + 7.5 + 5 + 5) / 5 = 6, c1 = 0.
    round 3  c = (6, 0).  x = 2.5: 12.25 to c0, 6.25 to c1: label 1.  labels 1 0 1 0 0 0, one change,
             distortion 0 + 16 + 6.25 + 2.25 + 1 + 1 = 26.5.  Update c0 = 27.5 / 4 = 6.875, c1 = 2.5 / 2 = 1.25.
    round 4  c = (6.875, 1.25).  Distances 1.5625, 9.765625, 1.5625, 0.390625, 3.515625, 3.515625 to the codewords
             of the same labels, no change, no empty cluster: the sub-space stops, no update.     (the stop rule decides)
             distortion 20.3125.
    So iters_run = 4, converged, one reseeded cluster, codebook (6.875, 1.25).  Limited to 3 rounds, the same codebook
    comes out of round 3's update, not converged."""
    cb, st = train(HAND_POINTS, 1, 2, 25, HAND_INIT)
    assert np.array_equal(cb, HAND_CODEBOOK), cb
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (4, 1, 1), st
    assert list(st["distortion"]) == HAND_DISTORTION, st["distortion"]
    cb, st = train(HAND_POINTS, 1, 2, 3, HAND_INIT)
    assert np.array_equal(cb, HAND_CODEBOOK), cb
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (3, 0, 1), st
    assert list(st["distortion"]) == HAND_DISTORTION[:3], st["distortion"]
    cb, st = train(HAND_POINTS, 1, 2, 1, HAND_INIT)
    assert np.array_equal(cb, np.array([[[5.0], [0.0]]], dtype=np.float32)), cb
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (1, 0, 1), st


def test_restatement_on_the_hand_derived_case():
    check_hand_case(lambda v, M, K, it, init: R.train(v, M, K, max_iters=it, init=init))
    lab, win = R.assign(HAND_POINTS, np.array([[5.0], [0.0]], dtype=np.float32))
    assert lab.tolist() == [1, 0, 0, 0, 0, 0] and win.tolist() == [0.0, 25.0, 6.25, 6.25, 0.0, 0.0]


def test_seeded_start_of_the_restatement():
    rows = R.seeded_rows(1000, 16, 5)
    assert len(set(rows)) == 16 and all(0 <= r < 1000 for r in rows)
    assert R.seeded_rows(1000, 16, 5) == rows and R.seeded_rows(1000, 16, 6) != rows
    # splitmix64's first output for state 0 is 0xE220A8397B1DCDAF: row 0 of a seed-0 draw
    assert R.seeded_rows(1000, 1, 0) == [0xE220A8397B1DCDAF % 1000]
    assert sorted(R.seeded_rows(16, 16, 1)) == list(range(16))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_distortion_does_not_increase(name):
    """The property the GPU test asserts, checked first on the restatement, for exactly the GPU test's inputs."""
    c, cb, st = case(name)
    assert_monotone(st["distortion"], cb.shape[2])
    if name == "g_stop":
        assert st["converged"] == 1 and st["iters_run"] < 64
    if name == "f_dups":
        assert st["reseeded"] >= 2 * 47


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def _gpu_train(gpu, c, max_iters=None):
    return gpu.train_codebook(c["vectors"], M=c["M"], K=c["K"], max_iters=max_iters or c["max_iters"], seed=c["seed"],
                              init=c["init"])


@pytest.mark.gpu
def test_gpu_hand_derived_case(gpu):
    check_hand_case(lambda v, M, K, it, init: gpu.train_codebook(v, M=M, K=K, max_iters=it, init=init))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_matches_the_restatement_bit_for_bit(gpu, name):
    c, ref_cb, ref = case(name)
    cb, st = _gpu_train(gpu, c)
    n, M = len(c["vectors"]), c["M"]
    print(name, "gpu", st["iters_run"], st["converged"], st["reseeded"], "ref", ref["iters_run"], ref["converged"], ref["reseeded"])
    assert (st["iters_run"], st["converged"], st["reseeded"]) == (ref["iters_run"], ref["converged"], ref["reseeded"])
    differing = int((cb.view(np.uint32) != ref_cb.view(np.uint32)).sum())
    assert differing == 0, "%d of %d codeword values differ from the restatement" % (differing, cb.size)
    assert len(st["distortion"]) == len(ref["distortion"])
    for r, (got, want) in enumerate(zip(st["distortion"], ref["distortion"])):
        print("round %d distortion gpu %.17g restatement %.17g" % (r + 1, got, want))
        assert abs(got - want) <= n * M * 2.0 ** -52 * want, (r, got, want)
    assert_monotone(st["distortion"], cb.shape[2])


@pytest.mark.gpu
def test_gpu_seeded_start_is_the_restated_one(gpu):
    """One round from the seeded start and the same round from the restated rows given as an initial codebook."""
    c, _, _ = case("a_init")
    v = c["vectors"]
    rows = R.seeded_rows(len(v), 64, 77)
    init = np.stack([s[rows] for s in R.split(v, 2)])
    a, _ = gpu.train_codebook(v, M=2, K=64, max_iters=1, seed=77)
    b, _ = gpu.train_codebook(v, M=2, K=64, max_iters=1, init=init)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
def test_gpu_run_twice_same_bytes(gpu):
    for name in ("b_real", "f_dups"):
        c, _, _ = case(name)
        a, sa = _gpu_train(gpu, c)
        b, sb = _gpu_train(gpu, c)
        assert a.tobytes() == b.tobytes()
        assert sa["distortion"] == sb["distortion"] and sa["reseeded"] == sb["reseeded"]


@pytest.mark.gpu
def test_gpu_labels_of_a_round_are_the_encoders(gpu):
    """Round r + 1 assigns with dpq_encode_pq's arithmetic: encoding the vectors with the codebook of an r-round run
    and applying the restated update to those labels gives the codebook of the (r + 1)-round run."""
    c, _, _ = case("b_real")
    r = 3
    before, _ = _gpu_train(gpu, c, max_iters=r)
    after, st = _gpu_train(gpu, c, max_iters=r + 1)
    assert st["iters_run"] == r + 1
    codes = gpu.encode_pq(c["vectors"], before)
    _, ref = R.train(c["vectors"], c["M"], c["K"], r + 1, c["seed"], c["init"])
    assert np.array_equal(codes, ref["labels"].astype(np.uint8))
    for m, sub in enumerate(R.split(c["vectors"], c["M"])):
        lab, win = R.assign(sub, before[m])
        assert np.array_equal(lab, codes[:, m])
        want, _ = R.update(sub, codes[:, m].astype(np.int64), win, before[m])
        assert np.array_equal(want.view(np.uint32), after[m].view(np.uint32))


@pytest.mark.gpu
def test_gpu_end_to_end_from_vectors_to_queries(gpu, oracle):
    from conftest import assert_parity, oracle_topk
    from deltapq_amd import synth
    n, k = 6000, 10
    base = synth.make_clustered_vectors(n, 128, seed=31, n_clusters=150, centre_seed=30)
    qs = synth.make_clustered_vectors(12, 128, seed=32, n_clusters=150, centre_seed=30)
    cb, st = gpu.train_codebook(base, M=8, K=256, max_iters=6, seed=1)
    assert st["iters_run"] == 6 and cb.shape == (8, 256, 16)
    codes = gpu.encode_pq(base, cb)
    tree = gpu.DeltaTree(codes, codebook=cb, device=0)
    payload = tree.payload()
    with gpu.DeltaPQIndex.open_memory(payload, n, 8, 256, device=0) as idx:
        idx.set_codebook(cb)
        ids, dists = idx.query_batch(qs, k)
    assert_parity(ids, dists, oracle_topk(oracle, payload, n, cb, qs, k), n)


@pytest.mark.gpu
def test_gpu_cli_chain_learn_encode_tree_query(gpu, oracle, tmp_path):
    from conftest import assert_parity, oracle_topk
    from deltapq_amd import synth
    d, n, nq, k = str(tmp_path), 5000, 10, 10
    learn = synth.make_clustered_vectors(7000, 128, seed=41, n_clusters=150, centre_seed=40)
    base = synth.make_clustered_vectors(n, 128, seed=42, n_clusters=150, centre_seed=40)
    qs = synth.make_clustered_vectors(nq, 128, seed=43, n_clusters=150, centre_seed=40)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), learn)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), qs)
    out = os.path.join(d, "results.bin")
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    for args in (["-task", "learn", "-N", "6000"], ["-task", "encode"],
                 ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"],
                 ["-task", "query", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-out", out]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr   # a failed step ends the chain
    cb = gpu.read_codewords(os.path.join(d, "M8K256codewords.txt"))
    want, st = gpu.train_codebook(learn[:6000], M=8, K=256)      # the CLI's defaults: 25 rounds, seed 0, a prefix for -N
    assert np.array_equal(cb.view(np.uint32), want.view(np.uint32))
    n_codes, payload = gpu.read_dtc_file(synth.dtc_file_name(d, 8, 256, n))
    assert n_codes == n
    raw = open(out, "rb").read()
    assert np.frombuffer(raw[:16], dtype=np.int64).tolist() == [nq, k]
    ids = np.frombuffer(raw[16:16 + nq * k * 4], dtype=np.int32).reshape(nq, k)
    dists = np.frombuffer(raw[16 + nq * k * 4:], dtype=np.float32).reshape(nq, k)
    assert_parity(ids, dists, oracle_topk(oracle, payload, n, cb, qs, k), n)
