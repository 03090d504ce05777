"""OPQ without a GPU: the Procrustes solver (dpq_procrustes), the rotation file, the argument checks of every OPQ entry,
and the self-checks of tests/_opq_restatement.py.  The GPU side is tests/test_opq.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _opq_restatement as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deltapq_amd", "csrc")
ERR_ARG, ERR_FORMAT = -1, -3
EPS = 2.0 ** -52
# Measured on the fixed matrices below (x86-64, g++ -O3 -ffp-contract=off; numpy with OpenBLAS LAPACK):
#   max |R^T R - I| is at most 0.95 * D * 2^-52 (D = 128: 2.69e-14), inside the stated 64 * D * 2^-52;
#   max |R - U V^T| against numpy.linalg.svd is at most 4.83e-15 (D = 128); the tolerance is 16 times that, the margin
#   being for LAPACK builds that differ.
SVD_TOL = 16 * 4.83e-15


def orth_bound(D):
    return 64 * D * EPS


def fixed_matrix(D):
    """P diag(s) Q^T from seeded orthogonal P, Q; s spread over one decade."""
    rng = np.random.default_rng(1000 + D)
    P = np.linalg.qr(rng.standard_normal((D, D)))[0]
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    s = np.logspace(0, 1, D)
    return P @ np.diag(s) @ Q.T


def degenerate_matrices():
    rng = np.random.default_rng(77)
    zero_row = rng.standard_normal((8, 8))
    zero_row[3] = 0.0
    with_inf = rng.standard_normal((4, 4))
    with_inf[1, 2] = np.inf
    return {"zero": np.zeros((5, 5)), "rank-1": np.outer(rng.standard_normal(6), rng.standard_normal(6)),
            "zero row": zero_row, "inf": with_inf}


@pytest.fixture(scope="module")
def api(lib):
    from deltapq_amd import api
    return api


def raw_procrustes(lib, C, fill=7.0):
    C = np.ascontiguousarray(C, dtype=np.float64)
    out = np.full_like(C, fill)
    deg = ctypes.c_int32(-1)
    rc = lib.dpq_procrustes(ctypes.c_void_p(C.ctypes.data), C.shape[0], ctypes.c_void_p(out.ctypes.data), deg)
    return rc, out, deg.value


# ---- Procrustes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [2, 3, 16, 128])
def test_procrustes_fixed_matrices(api, D):
    C = fixed_matrix(D)
    R, deg = api.procrustes(C)
    assert not deg
    orth = np.max(np.abs(R.T @ R - np.eye(D)))
    U, _, Vt = np.linalg.svd(C)
    diff = np.max(np.abs(R - U @ Vt))
    print("D = %d: |R^T R - I| = %.3g (%.3g D eps), |R - U V^T| = %.3g" % (D, orth, orth / (D * EPS), diff))
    assert orth <= orth_bound(D)
    assert diff <= SVD_TOL


def test_procrustes_exact_known_answers(api):
    rng = np.random.default_rng(3)
    perm = np.eye(7)[rng.permutation(7)]
    signed = perm * rng.choice([-1.0, 1.0], size=7)[None, :]
    for C, want in ((perm, perm), (signed, signed), (2.0 * np.eye(5), np.eye(5))):
        R, deg = api.procrustes(C)
        assert not deg
        assert R.tobytes() == np.ascontiguousarray(want + 0.0, dtype=np.float64).tobytes()
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s], [s, c]])
    R, deg = api.procrustes(5.0 * rot)
    assert not deg and np.max(np.abs(R - rot)) <= orth_bound(2)


@pytest.mark.parametrize("name", ["zero", "rank-1", "zero row", "inf"])
def test_procrustes_degenerate_inputs_leave_the_output_alone(lib, name):
    rc, out, deg = raw_procrustes(lib, degenerate_matrices()[name])
    assert rc == 0 and deg == 1
    assert np.all(out == 7.0)


def test_procrustes_is_deterministic(lib):
    C = fixed_matrix(16)
    a, b = raw_procrustes(lib, C), raw_procrustes(lib, C)
    assert a[2] == b[2] == 0 and a[1].tobytes() == b[1].tobytes()


# ---- rotation file -----------------------------------------------------------------------------------------------------

def test_rotation_file_round_trip(api, tmp_path):
    rng = np.random.default_rng(9)
    R = rng.standard_normal((6, 6)).astype(np.float32)
    R[0, 0], R[1, 2], R[2, 3] = np.float32(-0.0), np.float32(1e-42), np.float32(-1e-45)   # -0.0 and two denormals
    path = str(tmp_path / api.rotation_file_name("", 8, 256))
    assert os.path.basename(path) == "M8K256rotation.fvecs"
    api.write_rotation(path, R)
    assert os.path.getsize(path) == 6 * (4 + 4 * 6)
    assert api.read_rotation(path).tobytes() == R.tobytes()
    assert api.read_vecs(path).tobytes() == R.tobytes()      # the .fvecs layout


def test_rotation_file_refuses_truncated_and_non_square(api, lib, tmp_path):
    from deltapq_amd import synth
    R = np.eye(5, dtype=np.float32)
    good = str(tmp_path / "good.fvecs")
    api.write_rotation(good, R)
    raw = open(good, "rb").read()
    cut = str(tmp_path / "cut.fvecs")
    open(cut, "wb").write(raw[:-3])
    wide = str(tmp_path / "wide.fvecs")
    synth.write_fvecs(wide, np.ones((3, 5), dtype=np.float32))
    mixed = str(tmp_path / "mixed.fvecs")
    open(mixed, "wb").write(raw[:24] + np.int32(4).tobytes() + raw[28:])
    for bad in (cut, wide, mixed):
        with pytest.raises(api.DpqError) as e:
            api.read_rotation(bad)
        assert e.value.status == ERR_FORMAT, bad
    with pytest.raises(api.DpqError) as e:
        api.read_rotation(str(tmp_path / "absent.fvecs"))
    assert e.value.status == -2 and "absent.fvecs" in str(e.value)


# ---- argument errors, all before any device call ----------------------------------------------------------------------

def test_argument_errors_need_no_device(lib):
    from deltapq_amd import _lib
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    x = np.zeros((32, 8), dtype=np.float32)
    out = np.zeros_like(x)
    R = np.eye(8, dtype=np.float32)
    big = np.zeros((1, 4), dtype=np.float32)
    codes = np.zeros((32, 2), dtype=np.uint8)
    cb = np.zeros((2, 4, 4), dtype=np.float32)
    C = np.zeros((8, 8), dtype=np.float64)
    R64 = np.zeros((8, 8), dtype=np.float64)
    deg = ctypes.c_int32()
    fake = ctypes.c_void_p(0x1000)      # never dereferenced: the checks come first

    # dpq_rotate / dpq_rotate_device
    assert lib.dpq_rotate(None, 32, 8, vp(R), 0, vp(out)) == ERR_ARG
    assert lib.dpq_rotate(vp(x), 32, 8, None, 0, vp(out)) == ERR_ARG
    assert lib.dpq_rotate(vp(x), 32, 8, vp(R), 0, None) == ERR_ARG
    assert lib.dpq_rotate(vp(x), 32, 0, vp(R), 0, vp(out)) == ERR_ARG
    assert lib.dpq_rotate(vp(big), 1, 1025, vp(R), 0, vp(out)) == ERR_ARG
    assert lib.dpq_rotate(vp(x), -1, 8, vp(R), 0, vp(out)) == ERR_ARG
    assert lib.dpq_rotate(vp(x), 32, 8, vp(R), 0, vp(x)) == ERR_ARG and b"alias" in lib.dpq_last_error()
    assert lib.dpq_rotate_device(None, 32, 8, fake, fake, None) == ERR_ARG
    assert lib.dpq_rotate_device(fake, 32, 0, fake, ctypes.c_void_p(0x2000), None) == ERR_ARG
    assert lib.dpq_rotate_device(fake, 32, 1025, fake, ctypes.c_void_p(0x2000), None) == ERR_ARG
    assert lib.dpq_rotate_device(fake, 32, 8, ctypes.c_void_p(0x3000), fake, None) == ERR_ARG

    # dpq_cross_covariance
    assert lib.dpq_cross_covariance(None, 32, 8, vp(codes), vp(cb), 2, 4, 4, 0, vp(C)) == ERR_ARG
    assert lib.dpq_cross_covariance(vp(x), 32, 8, vp(codes), vp(cb), 2, 4, 4, 0, None) == ERR_ARG
    assert lib.dpq_cross_covariance(vp(x), 32, 0, vp(codes), vp(cb), 2, 4, 4, 0, vp(C)) == ERR_ARG
    assert lib.dpq_cross_covariance(vp(x), 32, 1025, vp(codes), vp(cb), 2, 4, 4, 0, vp(C)) == ERR_ARG
    assert lib.dpq_cross_covariance(vp(x), 32, 8, vp(codes), vp(cb), 2, 4, 3, 0, vp(C)) == ERR_ARG     # D != M * Ds
    assert lib.dpq_cross_covariance(vp(x), 0, 8, vp(codes), vp(cb), 2, 4, 4, 0, vp(C)) == ERR_ARG
    bad_codes = codes.copy()
    bad_codes[5, 1] = 4
    assert lib.dpq_cross_covariance(vp(x), 32, 8, vp(bad_codes), vp(cb), 2, 4, 4, 0, vp(C)) == ERR_ARG

    # dpq_procrustes
    assert lib.dpq_procrustes(None, 8, vp(R64), deg) == ERR_ARG
    assert lib.dpq_procrustes(vp(C), 8, None, deg) == ERR_ARG
    assert lib.dpq_procrustes(vp(C), 8, vp(R64), None) == ERR_ARG
    assert lib.dpq_procrustes(vp(C), 0, vp(R64), deg) == ERR_ARG
    assert lib.dpq_procrustes(vp(C), 1025, vp(R64), deg) == ERR_ARG

    # dpq_opq_train
    rot = np.zeros((8, 8), dtype=np.float32)
    cw = np.zeros((2, 4, 4), dtype=np.float32)

    def train(v=x, n=32, D=8, M=2, K=4, r=rot, c=cw, **o):
        opts = _lib.OpqOpts(device=0, outer_iters=2, init_iters=2, inner_iters=2)
        for k, val in o.items():
            setattr(opts, k, val)
        return lib.dpq_opq_train(vp(v) if v is not None else None, n, D, M, K, opts, vp(r) if r is not None else None,
                                 vp(c) if c is not None else None, None)

    assert train(v=None) == ERR_ARG and train(r=None) == ERR_ARG and train(c=None) == ERR_ARG
    assert train(D=0) == ERR_ARG and train(D=1025) == ERR_ARG
    assert train(M=3) == ERR_ARG and b"multiple of M" in lib.dpq_last_error()
    assert train(outer_iters=65) == ERR_ARG and train(outer_iters=-1) == ERR_ARG
    assert train(init_iters=0) == ERR_ARG and train(init_iters=65) == ERR_ARG
    assert train(inner_iters=0) == ERR_ARG and train(inner_iters=65) == ERR_ARG
    assert train(init=2) == ERR_ARG and train(restarts=17) == ERR_ARG
    assert train(K=1) == ERR_ARG and train(n=3) == ERR_ARG      # what dpq_train_codebook refuses

    # the rotation file
    assert lib.dpq_write_rotation(None, vp(R), 8) == ERR_ARG
    assert lib.dpq_write_rotation(b"/nonexistent-dir/x", None, 8) == ERR_ARG
    assert lib.dpq_write_rotation(b"/nonexistent-dir/x", vp(R), 0) == ERR_ARG
    assert lib.dpq_write_rotation(b"/nonexistent-dir/x", vp(R), 1025) == ERR_ARG
    assert lib.dpq_read_rotation(None, deg, None) == ERR_ARG
    assert lib.dpq_read_rotation(b"/nonexistent-dir/x", None, None) == ERR_ARG


def test_struct_layouts(lib):
    from deltapq_amd import _lib
    assert ctypes.sizeof(_lib.OpqOpts) == 4 * 4 + 8 + 4 * 4
    assert ctypes.sizeof(_lib.OpqStats) == 4 * 4 + (65 + 64) * 8 + 9 * 8


# ---- the restatement's own arithmetic ------------------------------------------------------------------------------------

def test_restatement_identity_and_permutation():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((50, 12)) * 2.0 ** rng.integers(-20, 20, size=(50, 12))).astype(np.float32)
    assert OR.rotate(x, np.eye(12, dtype=np.float32)).tobytes() == x.tobytes()
    p = rng.permutation(12)
    P = np.zeros((12, 12), dtype=np.float32)
    P[p, np.arange(12)] = 1.0           # out[:, j] = x[:, p[j]]
    assert OR.rotate(x, P).tobytes() == np.ascontiguousarray(x[:, p]).tobytes()


@pytest.mark.parametrize("x,col,want", OR.HAND_ROWS)
def test_restatement_hand_derived_rows(x, col, want):
    xv, R = OR.hand_row_case(x, col)
    out = OR.rotate(xv, R)
    assert out[0, 0].tobytes() == np.float32(want).tobytes()
    assert not out[0, 1:].any()


def test_restatement_leaf_rule_literal():
    x, codes, cb = OR.leaf_rule_case()
    C = OR.cross_covariance(x, codes, cb)
    assert C.shape == (1, 1) and C[0, 0] == 2.0 ** 60 + 256.0
    one_chain = 0.0
    for i in range(1280):
        one_chain = one_chain + float(x[i, 0]) * float(cb[0, codes[i, 0], 0])
    assert one_chain == 2.0 ** 60


# ---- the solver under the sanitizers ----------------------------------------------------------------------------------------

def test_procrustes_solver_under_sanitizers(lib, tmp_path):
    """tests/opq_procrustes_main.cpp + dpq_procrustes.cpp, g++ -fsanitize=address,undefined, run as a child process:
    exit status 0 and an empty stderr.  Nothing is preloaded; no GPU is involved: sanitizer runs belong on hosts
    without one, and a process environment that preloads a library would put it ahead of the sanitizer runtime."""
    if lib.dpq_device_count() > 0:
        pytest.skip("a GPU is present: the sanitizer run is for CPU-only hosts")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: a preloaded library would come ahead of the sanitizer runtime")
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "opq_procrustes_main")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "opq_procrustes_main.cpp"), os.path.join(CSRC, "dpq_procrustes.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    mats = [(fixed_matrix(D), 0) for D in (2, 3, 16, 128)] + [(m, 1) for m in degenerate_matrices().values()]
    path = str(tmp_path / "matrices.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(mats)).tobytes())
        for m, deg in mats:
            f.write(np.array([m.shape[0], deg], dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(m, dtype=np.float64).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
