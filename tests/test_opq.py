"""OPQ on the GPU: dpq_rotate / dpq_rotate_device and dpq_cross_covariance bit for bit against tests/_opq_restatement.py,
dpq_opq_train byte for byte against the loop of include/deltapq_amd.h written over the public calls, RotatedIndex and the
command line.  The host side (Procrustes, files, argument errors) is tests/test_opq_host.py."""
import os
import subprocess

import numpy as np
import pytest

import _opq_restatement as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deltapq_amd", "csrc", "deltapq")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(lib):
    from deltapq_amd import api
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path is the product and must be what runs here")
    return api


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def wide_vectors(rng, n, D):
    """fp32 values spanning 40 binades."""
    return (rng.standard_normal((n, D)) * 2.0 ** rng.integers(-20, 20, size=(n, D))).astype(np.float32)


def rotate_on_side_stream(gpu, x, R):
    """dpq_rotate_device on torch tensors, enqueued on a stream that is not the default one."""
    import torch
    xd, Rd = torch.from_numpy(x).cuda(), torch.from_numpy(R).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = gpu.rotate_torch(xd, Rd)
    side.synchronize()
    return out.cpu().numpy()


# ---- rotation ------------------------------------------------------------------------------------------------------------
# n = 2049 is beyond the issue's list: from 2048 rows on the launcher takes the kernel with four rows a lane.

@pytest.mark.parametrize("D", [1, 3, 4, 16, 96, 100, 128, 1024])
def test_rotate_matches_the_restatement(gpu, D):
    rng = np.random.default_rng(100 + D)
    R = rng.standard_normal((D, D)).astype(np.float32)      # not orthogonal: nothing cancels by luck
    for n in (1, 63, 64, 65) if D == 1024 else (1, 63, 64, 65, 257, 1000, 2049):
        x = wide_vectors(rng, n, D)
        want = bits(OR.rotate(x, R))
        assert np.array_equal(bits(gpu.rotate(x, R)), want), "host entry, n = %d" % n
        assert np.array_equal(bits(rotate_on_side_stream(gpu, x, R)), want), "device entry, n = %d" % n


def test_rotate_crosses_the_slice_boundary(gpu):
    n, D = (1 << 20) + 5, 4
    rng = np.random.default_rng(7)
    R = rng.standard_normal((D, D)).astype(np.float32)
    x = wide_vectors(rng, n, D)
    assert np.array_equal(bits(gpu.rotate(x, R)), bits(OR.rotate(x, R)))


@pytest.mark.parametrize("x,col,want", OR.HAND_ROWS)
def test_rotate_hand_derived_rows(gpu, x, col, want):
    xv, R = OR.hand_row_case(x, col)
    out = gpu.rotate(xv, R)
    assert out[0, 0].tobytes() == np.float32(want).tobytes()
    assert not out[0, 1:].any()


def test_rotate_device_unaligned_views_take_the_scalar_path(gpu):
    """A device pointer that is not 16-byte aligned (a view one float into a buffer) gives the same bits."""
    import torch
    rng = np.random.default_rng(11)
    n, D = 70, 8
    R = rng.standard_normal((D, D)).astype(np.float32)
    x = wide_vectors(rng, n, D)
    buf = torch.zeros(n * D + 1, dtype=torch.float32, device="cuda")
    obuf = torch.zeros(n * D + 1, dtype=torch.float32, device="cuda")
    xd = buf[1:].view(n, D)
    xd.copy_(torch.from_numpy(x))
    out = gpu.rotate_torch(xd, torch.from_numpy(R).cuda(), out=obuf[1:].view(n, D))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(OR.rotate(x, R)))


# ---- cross-covariance --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,M,K", [(8, 2, 4), (16, 4, 16), (128, 8, 256)])
def test_cross_covariance_matches_the_restatement(gpu, D, M, K):
    rng = np.random.default_rng(200 + D)
    cb = rng.standard_normal((M, K, D // M)).astype(np.float32)
    for n in (1, 1023, 1024, 1025, 2049, 5000):
        if D == 128 and n > 2049:
            continue
        x = rng.standard_normal((n, D)).astype(np.float32)
        codes = rng.integers(0, K, size=(n, M)).astype(np.uint8)
        got = gpu.cross_covariance(x, codes, cb)
        assert got.tobytes() == OR.cross_covariance(x, codes, cb).tobytes(), "n = %d" % n


def test_cross_covariance_leaf_rule_literal(gpu):
    x, codes, cb = OR.leaf_rule_case()
    C = gpu.cross_covariance(x, codes, cb)
    assert C.shape == (1, 1) and C[0, 0] == 2.0 ** 60 + 256.0      # one chain over all rows gives 2^60


# ---- the orthogonal case ------------------------------------------------------------------------------------------------------

def test_orthogonal_rotation_keeps_norms_and_inverts(gpu):
    """R = (float)R64, R64 orthogonal to about 1e-14.  Each entry of R carries one fp32 rounding, |E[d][j]| <= 2^-24 |R64[d][j]|,
    so |x . E| <= |x| * ||E||_F <= |x| * sqrt(D) * 2^-24; each output entry carries one more, relative 2^-24, hence 2^-24 on
    the norm.  Together (sqrt(D) + 1) * 2^-24 <= D * 2^-23 relative, for the norm and -- twice that, still inside for
    D >= 4 -- for the way there and back."""
    D, n = 64, 500
    rng = np.random.default_rng(21)
    R64, deg = gpu.procrustes(rng.standard_normal((D, D)))
    assert not deg
    R = R64.astype(np.float32)
    x = rng.standard_normal((n, D)).astype(np.float32)
    y = gpu.rotate(x, R)
    nx, ny = np.linalg.norm(x.astype(np.float64), axis=1), np.linalg.norm(y.astype(np.float64), axis=1)
    bound = D * 2.0 ** -23
    assert np.all(np.abs(ny - nx) <= bound * nx)
    back = gpu.rotate(y, np.ascontiguousarray(R.T))
    assert np.all(np.linalg.norm(back.astype(np.float64) - x, axis=1) <= bound * nx)


# ---- dpq_opq_train ------------------------------------------------------------------------------------------------------------

D_T, M_T, K_T = 16, 4, 16
OUTER, INIT_ITERS, INNER = 4, 4, 2


def correlated(n, z_seed=None):
    """(z . Q).astype(float32): Q orthogonal from default_rng(5), z Gaussian with per-dimension scale 0.8^d -- from the same
    generator (the issue's X), or from default_rng(z_seed): more rows of the same distribution."""
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.standard_normal((D_T, D_T)))[0]
    if z_seed is not None:
        rng = np.random.default_rng(z_seed)
    z = rng.standard_normal((n, D_T)) * 0.8 ** np.arange(D_T)
    return (z @ Q).astype(np.float32)


@pytest.fixture(scope="module")
def X():
    return correlated(2048)


def composed(gpu, X, start, rotation=None, seed=3):
    """The loop of include/deltapq_amd.h over the public calls."""
    D = X.shape[1]
    R = np.eye(D, dtype=np.float32) if rotation is None else np.array(rotation, dtype=np.float32)
    Xr = gpu.rotate(X, R)
    cb, _ = gpu.train_codebook(Xr, M=M_T, K=K_T, max_iters=INIT_ITERS, seed=seed, start=start, restarts=1)
    obj = [OR.objective(gpu.train_potential(Xr, cb))]
    best = (0, R.copy(), cb.copy())
    degenerate, residual = 0, []
    for t in range(1, OUTER + 1):
        codes = gpu.encode_pq(Xr, cb)
        C = gpu.cross_covariance(X, codes, cb)
        R64, deg = gpu.procrustes(C)
        if deg:
            degenerate += 1
        else:
            R = R64.astype(np.float32)
        residual.append(OR.orthogonality_residual(R))
        Xr = gpu.rotate(X, R)
        cb, _ = gpu.train_codebook(Xr, M=M_T, K=K_T, max_iters=INNER, init=cb)
        obj.append(OR.objective(gpu.train_potential(Xr, cb)))
        if obj[t] < obj[best[0]]:
            best = (t, R.copy(), cb.copy())
    return best, obj, degenerate, residual


@pytest.mark.parametrize("start,permuted", [("rows", False), ("kmeans++", False), ("rows", True)])
def test_opq_train_is_the_composition(gpu, X, start, permuted):
    rot0 = None
    if permuted:
        rot0 = np.zeros((D_T, D_T), dtype=np.float32)
        rot0[np.random.default_rng(8).permutation(D_T), np.arange(D_T)] = 1.0
    R, cb, st = gpu.train_opq(X, M=M_T, K=K_T, outer_iters=OUTER, init_iters=INIT_ITERS, inner_iters=INNER, seed=3, start=start,
                              rotation=rot0)
    (best_t, want_R, want_cb), obj, degenerate, _ = composed(gpu, X, start, rot0)
    assert st["outer_run"] == OUTER and st["best_t"] == best_t and st["degenerate"] == degenerate
    assert np.array(st["objective"]).tobytes() == np.array(obj).tobytes()
    assert R.tobytes() == want_R.tobytes() and cb.tobytes() == want_cb.tobytes()


def test_opq_train_without_outer_steps_is_train_codebook(gpu, X):
    R, cb, st = gpu.train_opq(X, M=M_T, K=K_T, outer_iters=0, init_iters=INIT_ITERS, inner_iters=INNER, seed=3)
    want, _ = gpu.train_codebook(X, M=M_T, K=K_T, max_iters=INIT_ITERS, seed=3)
    assert R.tobytes() == np.eye(D_T, dtype=np.float32).tobytes() and cb.tobytes() == want.tobytes()
    assert st["outer_run"] == 0 and st["best_t"] == 0 and len(st["objective"]) == 1


def test_opq_train_is_deterministic_and_does_what_it_is_for(gpu, X):
    args = dict(M=M_T, K=K_T, outer_iters=OUTER, init_iters=INIT_ITERS, inner_iters=INNER, seed=3)
    R, cb, st = gpu.train_opq(X, **args)
    R2, cb2, st2 = gpu.train_opq(X, **args)
    assert R.tobytes() == R2.tobytes() and cb.tobytes() == cb2.tobytes() and st["objective"] == st2["objective"]
    obj = st["objective"]
    print("objective per outer step:", obj, "best", st["best_t"])
    assert obj[st["best_t"]] < obj[0]
    plain, _ = gpu.train_codebook(X, M=M_T, K=K_T, max_iters=INIT_ITERS + OUTER * INNER, seed=3)
    plain_obj = OR.objective(gpu.train_potential(X, plain))
    print("plain PQ with the same rounds:", plain_obj)
    assert obj[st["best_t"]] < plain_obj
    # half an ulp (2^-24) per entry of a unit column, two columns, a factor two of margin
    assert len(st["rotation_residual"]) == OUTER
    assert all(r <= 4 * np.sqrt(D_T) * 2.0 ** -25 for r in st["rotation_residual"])
    assert OR.orthogonality_residual(R) <= 4 * np.sqrt(D_T) * 2.0 ** -25


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def recall_at(found, truth):
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / float(len(t)) for f, t in zip(found, truth)]))


def same_pair(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def check_rotated_index(gpu, idx, R, q, n):
    """RotatedIndex answers what the wrapped index answers for api.rotate(q, R), bit for bit."""
    import torch
    rq = gpu.rotate(q, R)
    ri = gpu.RotatedIndex(idx, R)
    assert same_pair(ri.query_batch(q, 10), idx.query_batch(rq, 10))
    with gpu.IdFilter.from_ids(idx, np.arange(0, n, 3)) as f:
        assert same_pair(ri.query_batch_filtered(q, 10, f), idx.query_batch_filtered(rq, 10, f))
    radius = float(np.median(idx.query_batch(rq, 10)[1][:, -1]))
    got, want = ri.range_search(q, radius), idx.range_search(rq, radius)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    assert want[0][-1] > 0
    ti, td = ri.query_batch_torch(torch.from_numpy(q).cuda(), 10)
    wi, wd = idx.query_batch_torch(torch.from_numpy(rq).cuda(), 10)
    torch.cuda.synchronize()
    assert same_pair((ti.cpu().numpy(), td.cpu().numpy()), (wi.cpu().numpy(), wd.cpu().numpy()))
    assert ri.info() == idx.info()            # everything else passes through
    return ri


def test_end_to_end_recall_and_rotated_index(gpu):
    """n = 4096, D = 16, K = 16, 64 queries of the same distribution, through the DeltaTree and the DTC index.  The issue
    states M = 4; every index of this library takes M = 8 or 16 only, so the sub-spaces here are M = 8 of two dimensions,
    everything else as stated."""
    n, nq, M = 4096, 64, 8
    Xb, q = correlated(n), correlated(nq, z_seed=99)
    outer, init_iters, inner = 8, 4, 2
    R, cb, _ = gpu.train_opq(Xb, M=M, K=K_T, outer_iters=outer, init_iters=init_iters, inner_iters=inner, seed=3)
    plain_cb, _ = gpu.train_codebook(Xb, M=M, K=K_T, max_iters=init_iters + outer * inner, seed=3)
    with gpu.FlatIndex(Xb) as flat:
        truth, _ = flat.search(q, 10)

    def opened(vectors, codebook):
        tree = gpu.DeltaTree(gpu.encode_pq(vectors, codebook), K=K_T, codebook=codebook, device=0)
        idx = gpu.DeltaPQIndex.open_memory(tree.payload(), n, M, K_T, device=0)
        idx.set_codebook(codebook)
        return tree, idx

    def recall_of(tree, searcher):
        pos = searcher.query_batch(q, 10)[0]
        pos = np.where(pos == n, n - 1, pos)        # even N: the id N names the last position
        return recall_at(tree.vec_id[pos], truth)

    tree, idx = opened(gpu.rotate(Xb, R), cb)
    with idx:
        opq_recall = recall_of(tree, check_rotated_index(gpu, idx, R, q, n))
    tree, idx = opened(Xb, plain_cb)
    with idx:
        pq_recall = recall_of(tree, idx)
    print("recall@10: PQ %.4f, OPQ %.4f" % (pq_recall, opq_recall))
    assert opq_recall > pq_recall


# ---- command line ----------------------------------------------------------------------------------------------------------------

def test_cli_chain_with_opq(gpu, tmp_path):
    from deltapq_amd import synth
    d, n, nq, k = str(tmp_path), 3000, 10, 5
    learn, base, qs = correlated(2048), correlated(n, z_seed=6), correlated(nq, z_seed=7)
    synth.write_fvecs(os.path.join(d, "learn.fvecs"), learn)
    synth.write_fvecs(os.path.join(d, "base.fvecs"), base)
    synth.write_fvecs(os.path.join(d, "query.fvecs"), qs)
    out = os.path.join(d, "results.bin")
    common = [EXE, "-dataset", d, "-m", "8", "-k", "256"]
    query = ["-task", "query", "-opq", "-N", str(n), "-query_size", str(nq), "-topk", str(k), "-out", out]

    def run(args):
        return subprocess.run(common + args, capture_output=True, text=True, timeout=300)

    r = run(["-task", "learn", "-opq", "2"])
    assert r.returncode == 0, r.stdout + r.stderr
    rot_path = gpu.rotation_file_name(d, 8, 256)
    R, cb, _ = gpu.train_opq(learn, M=8, K=256, outer_iters=2)         # the tool's defaults: 25 and 4 rounds, seed 0, rows
    assert gpu.read_rotation(rot_path).tobytes() == R.tobytes()
    assert gpu.read_codewords(os.path.join(d, "M8K256codewords.txt")).tobytes() == cb.tobytes()
    for args in (["-task", "encode", "-opq"], ["-task", "approx_tree", "-N", str(n), "-h", "1", "-diff", "8"], query):
        r = run(args)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr     # a failed step ends the chain
    codes = gpu.read_codes_plain(os.path.join(d, "codes.bin.plain.M8K256N%d" % n), 8)
    assert np.array_equal(codes, gpu.encode_pq(gpu.rotate(base, R), cb))
    raw = open(out, "rb").read()
    assert np.frombuffer(raw[:16], dtype=np.int64).tolist() == [nq, k]
    ids = np.frombuffer(raw[16:16 + nq * k * 4], dtype=np.int32).reshape(nq, k)
    dists = np.frombuffer(raw[16 + nq * k * 4:], dtype=np.float32).reshape(nq, k)
    with gpu.DeltaPQIndex.open_file(synth.dtc_file_name(d, 8, 256, n), 8, 256) as idx:
        idx.set_codebook(cb)
        assert same_pair((ids, dists), gpu.RotatedIndex(idx, R).query_batch(qs, k))
    # refusals: the refine level is out of scope, and a missing rotation file is named
    r = run(["-task", "refine", "-opq", "-N", str(n)])
    assert r.returncode == 2 and "usage" in r.stdout
    os.remove(rot_path)
    r = run(query)
    assert r.returncode != 0 and "M8K256rotation.fvecs" in r.stdout
