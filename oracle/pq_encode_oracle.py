"""oracle/pq_encode_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

CPU restatement of the reference's PQ encoder, PQTree::EncodePlain (/root/reference/pq_tree.cpp:215-237):
per sub-space the nearest codeword in fp32 -- `diff = v - c; dist += diff * diff` with separately rounded
multiply and add, dimensions in order, strict `<` so that the first minimum wins.  PARITY UNPINNED (see
dtc_oracle.cpp): written from reading the source; the reference cannot be built here (OpenCV).  The GPU encoder
(encode_pq_kernel) is compared with this bit for bit.

The full contract of dpq_encode_pq, beyond the shapes the reference is run with:

  padding     column m * Ds + d of a vector reads as 0.0f when it is >= D (short vectors are zero padded, pq.cpp:114-123);
              columns of `vectors` beyond M * Ds are ignored.
  selection   the reference's loop, not an argmin: `best = FLT_MAX, best_k = 0`, and k is taken only if
              `dist < best`.  A NaN distance is therefore never taken, and neither is +inf nor FLT_MAX itself.
  nothing     if no distance of a (vector, sub-space) is below FLT_MAX the code is 0.  The reference starts from
              `min_ks = -1` and asserts there (pq_tree.cpp:231); the product answers 0.

Denormals are kept (numpy does not flush them; the kernel's __fsub_rn / __fmul_rn / __fadd_rn do not either)."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def sub_vectors(vectors, m, Ds):
    """float32 [n][Ds]: sub-space m of every vector, zero padded where m * Ds + d >= D."""
    v = np.asarray(vectors, dtype=np.float32)
    n, D = v.shape
    sub = np.zeros((n, Ds), dtype=np.float32)
    lo, hi = m * Ds, min((m + 1) * Ds, D)
    if hi > lo:
        sub[:, :hi - lo] = v[:, lo:hi]
    return sub


def sub_distances(vectors, codebook, m):
    """float32 [n][K]: the encoder's distance of every vector to every codeword of sub-space m -- fp32 subtract, fp32
    multiply and fp32 add, each separately rounded, dimensions in order.  May hold inf and NaN."""
    cb = np.asarray(codebook, dtype=np.float32)
    _, K, Ds = cb.shape
    sub = sub_vectors(vectors, m, Ds)
    dist = np.zeros((len(sub), K), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for d in range(Ds):
            diff = (sub[:, d:d + 1] - cb[m, :, d][None, :]).astype(np.float32)
            dist = (dist + (diff * diff).astype(np.float32)).astype(np.float32)
    return dist


def select(dist):
    """The reference's selection over the last axis: the first k whose distance is below FLT_MAX and below every
    earlier one; 0 where there is none.  Vectorised: what `dist < FLT_MAX` refuses (NaN, inf, FLT_MAX) becomes +inf,
    argmin takes the first minimum, and a row that is all +inf answers 0 (the first of equals)."""
    dist = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        usable = dist < FLT_MAX
    return np.where(usable, dist, np.float32(np.inf)).argmin(-1)


def encode_pq(vectors, codebook):
    v = np.asarray(vectors, dtype=np.float32)
    cb = np.asarray(codebook, dtype=np.float32)
    M = cb.shape[0]
    codes = np.zeros((len(v), M), dtype=np.uint8)
    for m in range(M):
        codes[:, m] = select(sub_distances(v, cb, m))
    return codes
