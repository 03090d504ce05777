"""The OPQ arithmetic of include/deltapq_amd.h ("OPQ") in numpy: the GPU is held to this bit for bit.

Every multiply below is of two float32 values widened to float64, so the product is exact; every add is one
float64 add; the order is the stated one."""
import numpy as np

LEAF = 1024


def rotate(x, R):
    """out[i][j] = (float)(sum over d ascending, from +0.0 in fp64, of (double)x[i][d] * (double)R[d][j])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    R = np.ascontiguousarray(R, dtype=np.float32)
    n, D = x.shape
    assert R.shape == (D, D)
    acc = np.zeros((n, D), dtype=np.float64)
    x64, R64 = x.astype(np.float64), R.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(D):
            acc = acc + x64[:, d:d + 1] * R64[d][None, :]
        return acc.astype(np.float32)


def reconstruct(codes, codebook):
    """y[i][j] = codebook[j / Ds][codes[i][j / Ds]][j % Ds]."""
    M, K, Ds = codebook.shape
    return np.concatenate([codebook[m][codes[:, m]] for m in range(M)], axis=1)


def cross_covariance(x, codes, codebook):
    """C[d][j] = sum_i (double)x[i][d] * (double)y[i][j] by the leaf rule: S_l over a leaf's rows ascending from +0.0,
    T_0 = S_0, T_l = T_{l-1} + S_l."""
    x64 = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    y64 = reconstruct(np.asarray(codes), np.ascontiguousarray(codebook, dtype=np.float32)).astype(np.float64)
    n, D = x64.shape
    assert y64.shape == (n, D)
    T = None
    for lo in range(0, n, LEAF):
        S = np.zeros((D, D), dtype=np.float64)
        for i in range(lo, min(n, lo + LEAF)):
            S = S + x64[i][:, None] * y64[i][None, :]
        T = S if T is None else T + S
    return T


def objective(potential):
    """obj = the sum over m ascending, from +0.0, of the potential."""
    s = 0.0
    for p in np.asarray(potential, dtype=np.float64):
        s = s + float(p)
    return s


def orthogonality_residual(R):
    R64 = np.asarray(R, dtype=np.float64)
    return float(np.max(np.abs(R64.T @ R64 - np.eye(R64.shape[0]))))


# ---- hand-derived cases shared by tests/test_opq_host.py (the restatement) and tests/test_opq.py (the GPU) ----------

HAND_ROWS = [
    # (x, column 0 of R, expected out[0][0])
    ([2.0 ** 60, 1.0, -2.0 ** 60], [1.0, 1.0, 1.0], 0.0),       # 2^60 + 1 = 2^60 in fp64, then - 2^60
    ([2.0 ** 60, -2.0 ** 60, 1.0], [1.0, 1.0, 1.0], 1.0),       # ascending order: the cancellation comes first
    ([2.0 ** 24, 1.0, -2.0 ** 24], [1.0, 1.0, 1.0], 1.0),       # fp32 accumulation would give 0
    ([1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22], [1.0 + 2.0 ** -23, -1.0], 2.0 ** -46),  # a product rounded to fp32 would give 0
]


def hand_row_case(x, col):
    D = len(x)
    R = np.zeros((D, D), dtype=np.float32)
    R[:, 0] = col
    return np.array([x], dtype=np.float32), R


def leaf_rule_case():
    """n = 1280, D = M = 1, K = 2, codewords {2^30, 1}: C = 2^60 + 256 by leaves of 1024, 2^60 by one chain."""
    x = np.zeros((1280, 1), dtype=np.float32)
    codes = np.zeros((1280, 1), dtype=np.uint8)
    x[0, 0] = 2.0 ** 30
    x[1024:, 0] = 1.0
    codes[1024:, 0] = 1
    cb = np.array([[[2.0 ** 30], [1.0]]], dtype=np.float32)
    return x, codes, cb
